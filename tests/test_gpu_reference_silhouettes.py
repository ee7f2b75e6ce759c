"""GPU: the HIP path against the reference's own capture of Scene1 (tests/test_reference_silhouettes.py has the story; the fixture is
tests/golden/screenshot_silhouettes.json and nothing outside tests/golden is read).  The id scene at the capture's size, 1393 x 729,
one bounce: the frame kernels' image is the oracle's bit for bit AND its masks lie where the capture shows the objects — the second
holds on the HIP image alone, whatever the oracle does; the feature buffers (urt_render_aov) name the same object in every pixel; and
a mirrored camera axis or a horizontal field of view, traced by the library's own camera-ray code, is caught."""
import numpy as np
import pytest

import silhouette_ref as S
from unityraytracer_amd import RayTraceMaster

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sil():
    return S.silhouettes()


@pytest.fixture(scope="module")
def reference(oracle_lib):
    """(scene, ids, the oracle's frame) of the id scene, rendered once."""
    sc, ids = S.id_scene()
    frame, _ = S.oracle_ids(sc, mode=1)
    return sc, ids, frame


def hip_frame(ctx, sc, kernel_mode=3, frames_per_launch=0):
    ctx.set_option("kernel_mode", kernel_mode)
    ctx.set_option("frames_per_launch", frames_per_launch)
    try:
        m = RayTraceMaster(ctx, sc)
        m.OnRenderImage()
        got = m._target.GetPixels()
        m.OnDisable()
    finally:
        ctx.set_option("kernel_mode", 3)
        ctx.set_option("frames_per_launch", 0)
    return got


@pytest.mark.parametrize("kernel_mode,frames_per_launch", [(3, 0), (0, 0), (3, 1)])
def test_frame_kernels_put_the_objects_where_the_capture_shows_them(gpu_ctx, reference, sil, kernel_mode, frames_per_launch):
    sc, ids, ref = reference
    got = hip_frame(gpu_ctx, sc, kernel_mode, frames_per_launch)
    bad = int((got.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum())
    assert bad == 0, f"kernel_mode {kernel_mode}, frames_per_launch {frames_per_launch}: {bad} pixels differ from the oracle"
    m = S.measure(S.decode_ids(got), ids, sil)                                # the HIP image itself against the capture
    S.show(f"kernel_mode {kernel_mode} frames_per_launch {frames_per_launch}", m)
    S.assert_silhouettes(m, sil, f"kernel_mode {kernel_mode}")
    assert S.caught_by(m) == []


def aov_ids(aov, ids):
    """The id image (row 0 at the top) the feature buffers name: kind 2 / 3 with the object's index -> the id scene's id; ground and miss -> 0."""
    n_spheres = sum(kind == 2 for _, kind, _ in ids.values())
    out = np.where(aov["kind"] == 2, aov["object"] + 1, np.where(aov["kind"] == 3, aov["object"] + 1 + n_spheres, 0))
    return out[::-1].astype(np.int32)


def test_feature_buffers_name_the_object_the_frame_shows(gpu_ctx, reference, sil):
    """urt_render_aov against the emission image of the same context.  URT_AOV_FRAME_RAY traces the very ray of the frame: its kind and
    object give exactly the emission image's masks, for every object, the ground and the misses.  URT_AOV_PIXEL_CENTER cannot be equal
    in every pixel: the frame's ray is jittered — u = (x + rand + _PixelOffset.x) / width, RS:448 — so it passes up to one pixel right
    of and above the pixel's centre, inside the square of the four pixel centres (x .. x + 1, y .. y + 1).  A pixel where the two
    disagree has a silhouette through that square, so the pixel-centre id image is not constant over the pixel's 3 x 3 neighbourhood
    (every silhouette here is wider than a pixel).  Asserted: disagreement only there; every object's mask, the ground's and the
    misses' otherwise equal; and the capture's silhouette assertions on the pixel-centre image itself."""
    sc, ids, ref = reference
    m = RayTraceMaster(gpu_ctx, sc)
    m.Raycast((0, 1, 0), (0, 1, 0))                                           # binds the scene and frame 0's uniforms without rendering
    frame_ray = gpu_ctx.render_aov_arrays(sc.width, sc.height, frame_ray=True)
    centre = gpu_ctx.render_aov_arrays(sc.width, sc.height)
    m.Render()
    img = m._target.GetPixels()
    m.OnDisable()
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    shown = S.decode_ids(img)
    named = aov_ids(frame_ray, ids)
    for name, (k, _, _) in ids.items():
        assert np.array_equal(named == k, shown == k), name
    assert np.array_equal(named == 0, shown == 0)
    lit = img[::-1, :, 0] > 0
    assert np.array_equal(frame_ray["kind"][::-1] >= 2, lit)                  # ground (kind 1) and misses (kind 0) are the black pixels
    assert (frame_ray["kind"] == 0).any() and (frame_ray["kind"] == 1).any()
    assert np.array_equal(frame_ray["object"][::-1] == -1, ~lit)
    # pixel centres
    c = aov_ids(centre, ids)
    ck = centre["kind"][::-1]
    label = np.where(c > 0, c, -ck)                                           # objects by id, the ground -1, a miss 0: the horizon is a silhouette too
    pad = np.pad(label, 1, mode="edge")
    nb = np.stack([pad[1 + dy:1 + dy + c.shape[0], 1 + dx:1 + dx + c.shape[1]] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    edge = (nb != label[None]).any(axis=0)
    differ = c != shown
    print(f"pixel-centre ids differ from the frame's in {int(differ.sum())} pixels, {int(edge.sum())} pixels lie on a silhouette")
    assert not (differ & ~edge).any(), f"{int((differ & ~edge).sum())} pixels away from every silhouette name another object"
    assert 0 < differ.sum() < edge.sum()                                      # the jitter is there, and it is less than a pixel
    assert not ((ck == 0) != (frame_ray["kind"][::-1] == 0))[~edge].any() and not ((ck == 1) != (frame_ray["kind"][::-1] == 1))[~edge].any()
    mc = S.measure(c, ids, sil)
    S.show("pixel-centre feature buffers", mc)
    S.assert_silhouettes(mc, sil, "pixel-centre feature buffers", slack_pixels=1)       # its rays pass less than a pixel from the frame's


@pytest.mark.parametrize("variant", ["mirror_x", "horizontal_fov"])
def test_a_wrong_camera_is_caught_on_the_hip_path(gpu_ctx, sil, variant):
    """The variant's camera matrices go to the library as _CameraToWorld / _CameraInverseProjection: its own camera-ray code traces them.
    Either puts the off-centre pentagon elsewhere in the frame: the Cube (1) IoU catches it."""
    catcher = "Cube (1) IoU"
    sc, ids = S.id_scene(variant)
    got = hip_frame(gpu_ctx, sc)
    ref, _ = S.oracle_ids(sc, mode=1)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    m = S.measure(S.decode_ids(got), ids, sil)
    S.show(variant, m)
    caught = S.caught_by(m)
    assert catcher in caught, f"{variant}: not caught by {catcher} (Cube (1) IoU {m['iou']:.4f}; caught by {caught})"
    with pytest.raises(AssertionError):
        S.assert_silhouettes(m, sil, variant)
