"""Shared by tests/test_reference_silhouettes.py, tests/test_gpu_reference_silhouettes.py and tests/golden/make_silhouette_fixtures.py:
the "id scene" of the reference's Scene1 at the size of the reference's capture 25.64697-62.png, the statistics of a silhouette mask,
the comparison with what was mined from the capture (tests/golden/screenshot_silhouettes.json), and the negative variants — Scene1 as
a wrong reading of the reference's camera and object conventions would build it.

Id scene: scenes.from_unity_fixture of tests/golden/scene_Scene1.json without the objects the capture does not show, black sky, one
bounce, one ray, _PixelOffset (0.5, 0.5); every material has albedo = specular = 0 (Shade ends the path at the first hit) and emission
(k, 0, 0), k = 1, 2, ... in the order of object_ids: the frame's red channel IS the id of the first hit, 0 for the ground plane
and the sky.  All images here are indexed [row, x] with row 0 at the TOP (the capture's order); the library's and the oracle's frames
have row 0 at the bottom and are flipped by decode_ids.  Fractions of the frame: a box edge is first / size on the low side and
(last + 1) / size on the high side, a centroid is (mean + 0.5) / size."""
import copy
import json
import os

import numpy as np

from unityraytracer_amd import scenes

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WIDTH, HEIGHT = 1393, 729                                      # the capture's size: no resampling between it and the render
EDGES = ("left", "right", "top", "bottom")
ROUNDING = 1e-6                                                # the fixture's figures are written to six decimals
VARIANTS = ("mirror_x", "flip_rows", "horizontal_fov", "conjugate_quaternions", "transpose_matrices", "collider_radius")


def scene_fixture():
    return json.load(open(os.path.join(GOLD, "scene_Scene1.json")))


def silhouettes():
    return json.load(open(os.path.join(GOLD, "screenshot_silhouettes.json")))


def object_ids(fx, leave_out):
    """{name: (id, kind, index)} of the enabled objects kept: spheres first, then meshes, each in the fixture's order — the order of
    scenes.from_unity_fixture's _Spheres and _MeshObjects.  kind 2 = sphere, 3 = mesh (include/urt.h urt_RayHit.kind); index = the
    object's place in its list, what the feature buffers report as `object`."""
    kept = [o for o in fx["objects"] if o["enabled"] and o["name"] not in leave_out]
    sph, mesh = [o["name"] for o in kept if o["type"] == "sphere"], [o["name"] for o in kept if o["type"] != "sphere"]
    ids = {n: (1 + i, 2, i) for i, n in enumerate(sph)}
    ids.update({n: (1 + len(sph) + i, 3, i) for i, n in enumerate(mesh)})
    return ids


def id_scene(variant=None, leave_out=("Cube",)):
    """(scene, ids) — the id scene, or one negative variant of it.  Every variant changes what is handed to the oracle or the library
    (the fixture's numbers, the camera matrices, the MeshObjects), never the rendered image."""
    assert variant is None or variant in VARIANTS, variant
    fx = copy.deepcopy(scene_fixture())
    fx["objects"] = [o for o in fx["objects"] if o["name"] not in leave_out]
    for o in fx["objects"]:
        if variant == "conjugate_quaternions":                 # (x, y, z, w) -> (-x, -y, -z, w): the inverse rotation
            o["rotation"] = [-o["rotation"][0], -o["rotation"][1], -o["rotation"][2], o["rotation"][3]]
        if variant == "collider_radius" and o["type"] == "sphere":
            o["radius"] = o["collider_radius"]                 # SphereCollider.radius as it is, without the lossy scale (RO:33)
    sc = scenes.from_unity_fixture(fx, WIDTH, HEIGHT, sky=np.zeros((2, 4, 4), np.float32))
    sc.num_bounces, sc.num_rays, sc.pixel_offset, sc.seed = 1, 1, (0.5, 0.5), 0.5
    ids = object_ids(fx, leave_out)
    for name, (k, kind, index) in ids.items():
        lighting = (sc.spheres if kind == 2 else sc.mesh_objects)["lighting"]
        lighting["color_albedo"][index] = 0
        lighting["color_specular"][index] = 0
        lighting["emission"][index] = (k, 0, 0)
    c2w = np.array(sc.camera_to_world, np.float32)             # 16 floats, column-major: column j is [4j : 4j + 4]
    invp = np.array(sc.camera_inverse_projection, np.float64)
    if variant == "mirror_x":
        c2w[0:3] = -c2w[0:3]                                   # the camera's x axis points the other way
    if variant == "flip_rows":
        invp[4:8] = -invp[4:8]                                 # the projection's y negated: v = +1 is the bottom of the view
    if variant == "horizontal_fov":                            # tan(fov / 2) spans half the WIDTH: both extents shrink by the aspect ratio
        invp[0] = invp[0] * HEIGHT / WIDTH
        invp[5] = invp[5] * HEIGHT / WIDTH
    if variant == "transpose_matrices":
        m = sc.mesh_objects["localToWorldMatrix"].reshape(-1, 4, 4)
        sc.mesh_objects["localToWorldMatrix"] = np.ascontiguousarray(m.transpose(0, 2, 1)).reshape(-1, 16)
        sc.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(sc.mesh_objects, sc.vertices, sc.indices))
    sc.camera_to_world, sc.camera_inverse_projection = c2w, invp.astype(np.float32)
    return sc, ids


def decode_ids(frame):
    """(h, w, 4) frame with row 0 at the bottom -> (h, w) ids with row 0 at the top."""
    return np.rint(np.asarray(frame)[::-1, :, 0]).astype(np.int32)


def oracle_ids(sc, mode=1):
    """(frame, ids) of the scalar oracle; mode 0 = the literal loops, 1 = BVH-culled with its own triangle BVH."""
    from oracle import pyoracle
    o = pyoracle.Oracle(sc)
    if mode != 0:
        o.build_own_blas()
    frame = o.render(mode=mode, threads=8)
    return frame, decode_ids(frame)


def span_mask(spans, width=WIDTH, height=HEIGHT):
    """The mask of per-row [row, x_first, x_last] spans (one run per row)."""
    m = np.zeros((height, width), bool)
    for row, x0, x1 in spans:
        m[row, x0:x1 + 1] = True
    return m


def mask_stats(mask):
    """area, centroid (x, y) and box {left, right, top, bottom} of a mask as fractions of the frame; None for an empty mask."""
    h, w = mask.shape
    ys, xs = np.nonzero(mask)
    if len(xs) == 0:
        return None
    return {"area": len(xs) / (w * h), "centroid": [(xs.mean() + 0.5) / w, (ys.mean() + 0.5) / h],
            "box": {"left": xs.min() / w, "right": (xs.max() + 1) / w, "top": ys.min() / h, "bottom": (ys.max() + 1) / h}}


def iou(a, b):
    union = int((a | b).sum())
    return int((a & b).sum()) / union if union else 0.0


def measure(idimg, ids, sil):
    """Every figure the silhouette assertions use, of one id image against the mined fixture: the Cube (1) mask's IoU with the capture's
    span mask, its centroid's and box edges' distances, and for every mined edge of the other objects (error, tolerance).  An object
    that is not in the image at all has infinite errors."""
    cube_fx = sil["objects"]["Cube (1)"]
    mask = idimg == ids["Cube (1)"][0]
    st = mask_stats(mask)
    out = {"iou": iou(mask, span_mask(cube_fx["spans"], idimg.shape[1], idimg.shape[0])), "edges": {}}
    out["centroid"] = max(abs(a - b) for a, b in zip(st["centroid"], cube_fx["centroid"])) if st else np.inf
    out["cube_box"] = {e: abs(st["box"][e] - cube_fx["box"][e]) if st else np.inf for e in EDGES}
    for name, obj in sil["objects"].items():
        if name == "Cube (1)":
            continue
        st = mask_stats(idimg == ids[name][0])
        for e, rec in obj["edges"].items():
            out["edges"][(name, e)] = (abs(st["box"][e] - rec["value"]) if st else np.inf, rec["tolerance"])
    return out


def show(what, m):
    """Print every figure of measure() (tests print before they assert)."""
    print(f"{what}: Cube (1) IoU {m['iou']:.4f} centroid {m['centroid']:.4f} box " + " ".join(f"{e} {d:.4f}" for e, d in m["cube_box"].items()))
    print("   " + ", ".join(f"{n} {e} {d:.4f}/{tol:.4f}" for (n, e), (d, tol) in m["edges"].items()))


def assert_silhouettes(m, sil, what, slack_pixels=0):
    """The positive assertions: Cube (1) IoU / centroid / box, and every mined edge within its tolerance (+ slack_pixels of the edge's
    own axis, for an image whose rays are not the frame's: the tolerances were measured on the frame's)."""
    cube = sil["objects"]["Cube (1)"]
    assert m["iou"] >= cube["iou_bound"], (what, "Cube (1) IoU", m["iou"])
    assert m["centroid"] <= 0.002, (what, "Cube (1) centroid", m["centroid"])
    for e, d in m["cube_box"].items():
        assert d <= 0.006, (what, "Cube (1) box", e, d)
    for (name, e), (d, tol) in m["edges"].items():
        slack = slack_pixels / (sil["capture"]["width"] if e in ("left", "right") else sil["capture"]["height"])
        assert d <= tol + slack + ROUNDING, (what, name, e, d, tol)


def caught_by(m):
    """What catches a wrong image: 'Cube (1) IoU' when it is below 0.5, and every mined edge that is off by more than five times its
    tolerance, as 'name edge'."""
    out = ["Cube (1) IoU"] if m["iou"] < 0.5 else []
    return out + [f"{name} {e}" for (name, e), (d, tol) in m["edges"].items() if d > 5 * tol + ROUNDING]
