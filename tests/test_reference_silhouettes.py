"""The camera and object conventions pinned on something the reference itself produced: its capture 25.64697-62.png of Scene1.unity,
mined for the silhouettes of its objects (tests/golden/screenshot_silhouettes.json, written by tests/golden/make_silhouette_fixtures.py).
The oracle renders Scene1 as an id image at the capture's own size (tests/silhouette_ref.py) and the masks must lie where the capture
shows the objects: the black pentagon Cube (1) by IoU, centroid and box, the capsule, the cylinder and the spheres by the box edges
that segment reliably.  Kernel and oracle share one reading of the reference's camera ray, object transforms and sphere radii; a
mistake in that reading passes every bit-for-bit comparison between them and fails here — each negative variant below (mirrored x,
flipped rows, horizontal field of view, conjugated quaternions, transposed matrices, unscaled sphere radius) is rendered and must be
caught.  Geometry only: the capture's sky (.hdr) is not in the reference's tree, so radiance stays unpinned.  CPU only; the HIP path
is tests/test_gpu_reference_silhouettes.py."""
import json
import os
import sys

import numpy as np
import pytest

import silhouette_ref as S
from png_ref import read_png
from unityraytracer_amd import host_io

sys.path.insert(0, S.GOLD)
import make_silhouette_fixtures as mk  # noqa: E402  (the miner beside the fixtures; it imports PIL and scipy only when it mines)

# what must catch each variant, from the geometry: a mirrored or flipped camera puts the off-centre pentagon on the other side of the
# frame; a horizontal field of view magnifies the view about its centre by the aspect ratio 1.91; a transposed matrix loses its
# translation; a conjugated quaternion turns the 2 x 1 x 2 cylinder the other way about its own centre; and without the lossy scale
# Sphere (1) has half its radius.
CATCHERS = {"mirror_x": "Cube (1) IoU", "flip_rows": "Cube (1) IoU", "horizontal_fov": "Cube (1) IoU", "transpose_matrices": "Cube (1) IoU",
            "conjugate_quaternions": "Cylinder left", "collider_radius": "Sphere (1) top"}


@pytest.fixture(scope="module")
def sil():
    return S.silhouettes()


@pytest.fixture(scope="module")
def rendered(oracle_lib):
    """The id scene through the oracle's literal loops (mode 0) and its BVH-culled ones (mode 1): {mode: (frame, ids)}, rendered once."""
    sc, ids = S.id_scene()
    return sc, ids, {mode: S.oracle_ids(sc, mode) for mode in (0, 1)}


def test_fixture_says_what_it_was_mined_from(sil):
    assert sil["capture"] == {"name": "25.64697-62.png", "width": S.WIDTH, "height": S.HEIGHT}
    assert [o["name"] for o in sil["not_in_capture"]] == ["Cube"] and all(o["reason"] for o in sil["not_in_capture"] + sil["only_in_capture"])
    assert sorted(o["name"] for o in sil["only_in_capture"]) == ["Sphere (2)", "Sphere (5)"]
    cube = sil["objects"]["Cube (1)"]
    rows = [r for r, _, _ in cube["spans"]]
    assert rows == list(range(rows[0], rows[-1] + 1)) and all(a <= b for _, a, b in cube["spans"])         # one run in every row, no gap
    st = S.mask_stats(S.span_mask(cube["spans"]))
    assert st["area"] == pytest.approx(cube["area"], abs=S.ROUNDING) and st["centroid"] == pytest.approx(cube["centroid"], abs=S.ROUNDING)
    assert all(st["box"][e] == pytest.approx(cube["box"][e], abs=S.ROUNDING) for e in S.EDGES)
    sweep = cube["iou_with_oracle_over_sweep"]
    assert cube["iou_bound"] == (0.95 if max(sweep) - min(sweep) <= 0.01 else pytest.approx(min(sweep) - 0.01, abs=S.ROUNDING))
    assert set(sil["objects"]) >= {"Cube (1)", "Capsule", "Cylinder", "Sphere (1)"}
    assert set(sil["objects"]["Capsule"]["edges"]) == set(S.EDGES) and all(r["tolerance"] == 0.015 for r in sil["objects"]["Capsule"]["edges"].values())
    for name, obj in sil["objects"].items():
        if name in ("Cube (1)", "Capsule"):
            continue
        for e, r in obj["edges"].items():                                      # twice the measured difference, never above 0.01, stable in the sweep
            assert r["tolerance"] == pytest.approx(2 * r["difference"], abs=2 * S.ROUNDING) and r["tolerance"] <= 0.01, (name, e)
            assert r["difference"] == pytest.approx(abs(r["value"] - r["oracle"]), abs=2 * S.ROUNDING), (name, e)
            assert r["spread_over_sweep"] <= sil["stable_spread"], (name, e)
    for d in sil["dropped_edges"]:
        assert d["edge"] not in sil["objects"].get(d["object"], {"edges": {}})["edges"]
        assert d["reason"].startswith("clipped") or d["spread_over_sweep"] > sil["stable_spread"] or d["difference"] > sil["max_difference"], d


@pytest.mark.parametrize("mode", [0, 1])
def test_silhouettes_lie_where_the_capture_shows_them(rendered, sil, mode):
    sc, ids, out = rendered
    frame, idimg = out[mode]
    assert np.array_equal(frame[..., 0], np.rint(frame[..., 0])) and not frame[..., 1:3].any() and (frame[..., 3] == 1).all()
    assert set(np.unique(idimg).tolist()) == {0} | {k for k, _, _ in ids.values()}                        # every object is seen; 0 = ground and sky
    m = S.measure(idimg, ids, sil)
    S.show(f"oracle mode {mode}", m)
    S.assert_silhouettes(m, sil, f"oracle mode {mode}")
    assert S.caught_by(m) == []


def test_the_two_oracle_modes_render_the_same_ids(rendered):
    _, _, out = rendered
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))


@pytest.mark.parametrize("variant", S.VARIANTS)
def test_a_wrong_convention_is_caught(oracle_lib, sil, variant):
    sc, ids = S.id_scene(variant)
    _, idimg = S.oracle_ids(sc, mode=1)
    m = S.measure(idimg, ids, sil)
    S.show(variant, m)
    caught = S.caught_by(m)
    assert CATCHERS[variant] in caught, f"{variant}: not caught by {CATCHERS[variant]} (Cube (1) IoU {m['iou']:.4f}; caught by {caught})"
    if variant == "collider_radius":                                          # Sphere (1) is the sphere whose lossy scale is 2: every mined edge of it
        assert all(f"Sphere (1) {e}" in caught for e in sil["objects"]["Sphere (1)"]["edges"]), caught
    with pytest.raises(AssertionError):
        S.assert_silhouettes(m, sil, variant)


def test_screenshot_writer_keeps_the_captures_row_order(built_library, rendered, sil, tmp_path):
    """urt_host_write_png (what CaptureScreenshot, RM:762, writes) of the oracle's id image: the file's rows, decoded here with zlib, hold
    Cube (1) in the rows and columns of the capture's spans — PNG row 0 is the TOP of the view."""
    _, ids, out = rendered
    frame, idimg = out[1]
    n = max(k for k, _, _ in ids.values())
    shot = np.zeros_like(frame)
    shot[..., 0] = frame[..., 0] / np.float32(n)                               # ids as distinct greys in [0, 1]: the writer clamps above 1
    shot[..., 3] = 1
    path = str(tmp_path / "ids.png")
    host_io.write_png(path, shot)
    px = read_png(path)[4]
    assert px.shape == (S.HEIGHT, S.WIDTH, 3)
    table = np.zeros((n + 1, 1, 4), np.float32)
    table[:, 0, 0] = np.arange(n + 1, dtype=np.float32) / np.float32(n)
    codes = host_io.encode_srgb8(table)[:, 0, 0]
    assert len(set(codes.tolist())) == n + 1
    cube = px[..., 0] == codes[ids["Cube (1)"][0]]
    assert np.array_equal(cube, idimg == ids["Cube (1)"][0])                  # the file's rows are the view's, top first
    spans = S.span_mask(sil["objects"]["Cube (1)"]["spans"])
    assert S.iou(cube, spans) >= sil["objects"]["Cube (1)"]["iou_bound"]
    assert S.iou(cube[::-1], spans) < 0.5                                     # and the other row order is nowhere near
    rows = np.nonzero(cube.any(axis=1))[0]
    fx_rows = [r for r, _, _ in sil["objects"]["Cube (1)"]["spans"]]
    assert abs(rows[0] - fx_rows[0]) <= 0.006 * S.HEIGHT and abs(rows[-1] - fx_rows[-1]) <= 0.006 * S.HEIGHT


def test_fixture_regenerates_identically(oracle_lib, sil):
    """With the reference's tree at hand: mining its capture again gives the committed JSON."""
    path = os.path.join(mk.reference_root(), "Screenshots", mk.CAPTURE)
    if not os.path.exists(path):
        pytest.skip("the reference's tree is not on this machine")
    pytest.importorskip("PIL")
    pytest.importorskip("scipy")
    assert json.loads(json.dumps(mk.mine(path), sort_keys=True)) == sil
