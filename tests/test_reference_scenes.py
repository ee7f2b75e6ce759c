"""The reference's OWN scenes as fixtures: tests/golden/scene_Scene1.json and scene_SampleScene.json are
mined from Assets/Scenes/*.unity by tests/golden/make_scene_fixtures.py (camera, numBounces / numRays, every enabled RayTraceObject
with its transform, collider radius and material); Unity's built-in meshes are synthesised (scenes.unity_builtin_mesh), the sky is
procedural (the .hdr blobs are not in the reference's tree).  Radiance parity stays UNPINNED — no reference output with a known sky
exists for these scenes (where the objects stand IS pinned, on the capture of Scene1: tests/test_reference_silhouettes.py) — but the
configurations the reference's authors actually ran are exercised: Scene1.unity:1777-1779,1804-1805,1826-1827
(camera (0,1,-10), fov 81, numBounces 2, numRays 1, 6 spheres + 4 meshes) and SampleScene.unity:386,411-412,433-434 (camera pitched
10 degrees at (0,30,-80), fov 60, numBounces 10 x numRays 25).  CPU part: the fixtures, the stand-in meshes, and the qualitative
checks SURVEY §4 lists against statistics of the reference's screenshots (tests/golden/screenshot_stats.json)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle
from unityraytracer_amd import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def fixture(name):
    return json.load(open(os.path.join(GOLD, f"scene_{name}.json")))


def test_fixtures_hold_what_the_scene_files_say():
    s1, s2 = fixture("Scene1"), fixture("SampleScene")
    assert s1["numBounces"] == 2 and s1["numRays"] == 1                      # Scene1.unity:1826-1827
    assert s1["camera"]["position"] == [0, 1, -10] and s1["camera"]["field_of_view"] == 81
    en = [o for o in s1["objects"] if o["enabled"]]
    assert sum(o["type"] == "sphere" for o in en) == 6 and sum(o["type"] == "mesh" for o in en) == 4
    assert sorted(o["mesh"] for o in en if o["type"] == "mesh") == ["capsule", "cube", "cube", "cylinder"]
    assert len(s1["objects"]) - len(en) == 4                                  # the four disabled components never register (RO:22,46)
    big = next(o for o in en if o["name"] == "Sphere (1)")
    assert big["radius"] == pytest.approx(0.5 * 2.0)                         # RO:33: collider radius x largest lossy scale
    assert s2["numBounces"] == 10 and s2["numRays"] == 25                    # SampleScene.unity:433-434
    assert s2["camera"]["position"] == [0, 30, -80] and s2["camera"]["field_of_view"] == 60
    assert sorted(round(o["radius"], 3) for o in s2["objects"] if o["type"] == "sphere") == [7.5, 10.0, 10.0]
    assert all(o["albedoColor"] == [0.0, 0.4, 1.0] and o["smoothness"] == 0.69 for o in s2["objects"])    # script defaults, RO:12-15


def scene_yaml(fx, rto_guid, builtin_meshes):
    """Unity scene YAML (the serialisation mine() reads) of a fixture: one GameObject + Transform per object with its MeshFilter,
    SphereCollider and RayTraceObject MonoBehaviour (colour fields only when the fixture says they were serialised), and the camera
    with its Camera and the RayTraceMaster MonoBehaviour.  Written here from the fixture, so the round trip needs no scene file."""
    mesh_ids = {v: k for k, v in builtin_meshes.items()}
    lines, ids = ["%YAML 1.1", "%TAG !u! tag:unity3d.com,2011:"], iter(range(1000, 100000))
    vec = lambda v, keys="xyzw": "{" + ", ".join(f"{k}: {x!r}" for k, x in zip(keys, v)) + "}"

    def doc(cls, kind, fields):
        fid = next(ids)
        lines.extend([f"--- !u!{cls} &{fid}", f"{kind}:"] + [f"  {k}: {v}" for k, v in fields])
        return fid

    def game_object(name, pos, rot, scale):
        go = doc(1, "GameObject", [("m_Name", name), ("m_IsActive", 1)])
        doc(4, "Transform", [("m_GameObject", f"{{fileID: {go}}}"), ("m_LocalRotation", vec(rot)), ("m_LocalPosition", vec(pos)),
                             ("m_LocalScale", vec(scale)), ("m_Father", "{fileID: 0}")])
        return f"{{fileID: {go}}}"

    for o in fx["objects"]:
        go = game_object(o["name"], o["position"], o["rotation"], o["scale"])
        doc(33, "MeshFilter", [("m_GameObject", go), ("m_Mesh", f"{{fileID: {mesh_ids[o['mesh']]}, guid: 0000000000000000e000000000000000, type: 0}}")])
        if o["type"] == "sphere":
            doc(135, "SphereCollider", [("m_GameObject", go), ("m_Radius", repr(o["collider_radius"]))])
        mb = [("m_GameObject", go), ("m_Enabled", int(o["enabled"])), ("m_Script", f"{{fileID: 11500000, guid: {rto_guid}, type: 3}}")]
        if o["serialized_material"]:
            mb += [(c, vec(o[c] + [1.0], "rgba")) for c in ("albedoColor", "specularColor", "emissionColor")] + [("smoothness", repr(o["smoothness"]))]
        doc(114, "MonoBehaviour", mb)
    cam = fx["camera"]
    go = game_object("Main Camera", cam["position"], cam["rotation"], (1, 1, 1))
    doc(20, "Camera", [("m_GameObject", go), ("near clip plane", repr(cam["near"])), ("far clip plane", repr(cam["far"])),
                       ("field of view", repr(cam["field_of_view"]))])
    doc(114, "MonoBehaviour", [("m_GameObject", go), ("m_Enabled", 1), ("m_Script", "{fileID: 11500000, guid: 0123456789abcdef0123456789abcdef, type: 3}"),
                               ("numBounces", fx["numBounces"]), ("numRays", fx["numRays"])])
    return "\n".join(lines) + "\n"


def test_fixtures_regenerate_identically(tmp_path):
    """The committed script mines exactly the committed JSON back from scene YAML that holds the same scene (written from the
    fixture, above): its YAML reader, component grouping, sphere radius and material defaults agree with the fixtures."""
    sys.path.insert(0, GOLD)
    import make_scene_fixtures as mk
    guid = "fedcba9876543210fedcba9876543210"
    for name in ("Scene1", "SampleScene"):
        path = tmp_path / f"{name}.unity"
        path.write_text(scene_yaml(fixture(name), guid, mk.BUILTIN_MESHES))
        again = mk.mine(str(path), guid)
        assert json.loads(json.dumps(again, sort_keys=True)) == fixture(name)


def test_unity_builtin_mesh_stand_ins():
    for kind, tris, lo, hi in (("cube", 12, (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), ("cylinder", 80, (-0.5, -1, -0.5), (0.5, 1, 0.5)),
                               ("capsule", 832, (-0.5, -1, -0.5), (0.5, 1, 0.5)), ("quad", 2, (-0.5, -0.5, 0), (0.5, 0.5, 0)),
                               ("plane", 200, (-5, 0, -5), (5, 0, 5)), ("sphere", 768, (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))):
        v, t = scenes.unity_builtin_mesh(kind)
        assert len(t) == tris and t.min() == 0 and t.max() == len(v) - 1
        assert np.allclose(v.min(axis=0), lo, atol=0.01) and np.allclose(v.max(axis=0), hi, atol=0.01)
        if kind not in ("quad", "plane"):                                    # closed and consistently wound: every edge once in each direction
            e = {}
            for a, b, c in t:
                for p, q in ((a, b), (b, c), (c, a)):
                    e[(int(p), int(q))] = e.get((int(p), int(q)), 0) + 1
            assert all(n == 1 and (q, p) in e for (p, q), n in e.items()), kind


def render_mean(sc, frames):
    o = pyoracle.Oracle(sc)
    o.build_own_blas()
    acc = np.zeros((sc.height, sc.width, 4), np.float32)
    for i in range(frames):
        ox, oy, sd = scenes.frame_uniforms(i)
        o.set_frame((ox, oy), sd)
        acc = pyoracle.accumulate(o.render(mode=1, threads=8), acc, i)
    return acc


def test_scene1_looks_like_the_reference_screenshots():
    """Qualitative only: the captures are 8-bit, of unknown edit state and lit by an .hdr sky that is not in the tree.
    What must agree: the y = 0 plane's hard-coded colour (RS:167: albedo 0.5, 0.3, 0.15 -> r > g > b in the same proportions
    whatever lights it), the horizon at mid-height for Scene1's level camera, sky visible above it (energy is read BEFORE Shade
    zeroes it: A.3), and the cube rotated about all three axes rendering dark from object-space normals (A.6)."""
    stats = json.load(open(os.path.join(GOLD, "screenshot_stats.json")))
    shot = stats["25.64697-62.png"]                                          # the capture whose composition is Scene1's
    sc = scenes.from_unity_fixture(fixture("Scene1"), 348, 182)
    img = render_mean(sc, 12)                                                # row 0 = bottom
    h = sc.height
    ground, sky = img[: h // 4, :, :3].mean(axis=(0, 1)), img[3 * h // 4:, :, :3].mean(axis=(0, 1))
    assert ground[0] > ground[1] > ground[2] and shot["ground_mean_rgb"][0] > shot["ground_mean_rgb"][1] > shot["ground_mean_rgb"][2]
    # ground / sky per channel, relative to red = the plane's albedo ratios 0.3/0.5, 0.15/0.5 whatever the sky's colour is (ours
    # is a blue procedural sky, theirs a sunset .hdr); the 8-bit captures are display-encoded: linearised with gamma 2.2
    ours = (ground / sky) / (ground / sky)[0]
    for cap in stats.values():
        g, k_ = np.array(cap["ground_mean_rgb"]) ** 2.2, np.array(cap["sky_mean_rgb"]) ** 2.2
        theirs = (g / k_) / (g / k_)[0]
        assert np.allclose(theirs[1:], (0.6, 0.3), atol=0.12), (cap, theirs)
    assert np.allclose(ours[1:], (0.6, 0.3), atol=0.06), ours
    assert sky.mean() > 2.0 * ground.mean() > 0                              # the sky is seen, and it is what lights the plane
    lum = img[..., :3].mean(axis=(1, 2))[::-1]                               # per row, top to bottom
    k = 3
    drop = np.array([lum[y - k:y].mean() - lum[y:y + k].mean() for y in range(k, h - k)])
    assert abs((int(np.argmax(drop)) + k) / h - shot["ground_starts_at_row_fraction"]) < 0.03                 # 0.50 in both
    # the capture's black pentagon is Cube (1), the 1.12 x 2.06 x 1.38 mirror cube rotated about all three axes (its spans are mined in
    # tests/golden/screenshot_silhouettes.json; the geometry is pinned in tests/test_reference_silhouettes.py): black there, dark here
    # inside the capture's own mask, sampled at this render's pixel centres (rows of the mask run top-down)
    spans = json.load(open(os.path.join(GOLD, "screenshot_silhouettes.json")))
    mask = np.zeros((spans["capture"]["height"], spans["capture"]["width"]), bool)
    for row, x0, x1 in spans["objects"]["Cube (1)"]["spans"]:
        mask[row, x0:x1 + 1] = True
    ys = ((np.arange(h) + 0.5) / h * mask.shape[0]).astype(int)
    xs = ((np.arange(sc.width) + 0.5) / sc.width * mask.shape[1]).astype(int)
    inside = mask[np.ix_(ys, xs)][::-1]                                      # row 0 = bottom, like img
    assert inside.sum() > 1000
    pentagon = img[inside][:, :3].mean()
    assert pentagon < 0.5 * sky.mean(), (pentagon, sky.mean())               # measured: 0.097 against a sky mean of 0.61
    # the small rotated cube 1.3 units in front of the camera (not in the capture: it shows sky there) renders dark as well
    cube = next(o for o in fixture("Scene1")["objects"] if o["name"] == "Cube")
    assert cube["enabled"] and max(abs(c) for c in cube["rotation"][:3]) > 0.01
    o = pyoracle.Oracle(sc)
    o.build_own_blas()
    first = o.render(mode=1, threads=8)
    # project the cube's centre: camera at (0,1,-10) looking down +z, vertical fov 81
    dx, dy, dz = cube["position"][0] - 0.0, cube["position"][1] - 1.0, cube["position"][2] + 10.0
    f = 1.0 / np.tan(np.radians(81.0) / 2)
    px = int((dx / dz * f / (sc.width / sc.height) * 0.5 + 0.5) * sc.width)
    py = int((dy / dz * f * 0.5 + 0.5) * sc.height)
    patch = first[py - 3:py + 4, px - 3:px + 4, :3].mean()
    assert patch < 0.5 * sky.mean(), (patch, sky.mean())


def test_sample_scene_settings_run_on_the_oracle():
    """numBounces 10 x numRays 25 with the pitched camera: the literal loops (mode 0, no triangle BVH) and the BVH-culled ones agree."""
    sc = scenes.from_unity_fixture(fixture("SampleScene"), 64, 36)
    assert sc.num_bounces == 10 and sc.num_rays == 25
    o = pyoracle.Oracle(sc)
    o.build_own_blas()
    a, b = o.render(mode=0, threads=8), o.render(mode=1, threads=8)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isfinite(a).all() and a[..., :3].max() > 0.1 and (a[..., 3] == 1).all()
