"""GPU: option "front_fuse" of the scheduled trace kernel (csrc/kernels.hip k_sched, plain object-level phase: front modes 0 and 1).
With it on (the default) a new ray takes its first object-level step in the trip that created it; a scene of one heap node and no
spheres takes that step as straight-line code (csrc/front_device.h front_single).  Only WHEN a lane runs its operations changes, so
frames of 96 x 64 or smaller, four frames in one launch, kernel mode 3: front_fuse 1 == front_fuse 0 == the oracle, bit for bit, the
traced frame and the accumulated image —
  * reduced C3 (one blob: the straight-line form), also with 3 rays per pixel (the next ray is a new ray inside SHADE), with one
    bounce (every lane dies in its first SHADE trip: no step may run for it), with a material whose roulette ends paths, at both
    extreme threshold sets of tests/test_gpu_parity.py, and at frame shapes 1 x 1, 65 x 3 and 7 x 130 (ragged tiles in every frame);
  * the same blob with spheres, and the mixed scene with the BVH top outside FRONT: the general walk of front mode 0, which resumes;
  * two blobs with "front_list" 0: front mode 1, the BVH top walked inside the step;
and with count_stats the counters of the fused schedule equal the oracle's, `rays` included."""

import functools

import numpy as np
import pytest

from oracle import pyoracle
from unityraytracer_amd import RayTraceMaster, UrtError, scenes

pytestmark = pytest.mark.gpu

FRAMES = 4
RESTORE = {"front_fuse": -1, "count_stats": 0, "kernel_mode": 3, "front_list": -1, "top_front": -1, "refill_min": 16, "blas_min": 0,
           "blas_exit": 0, "shade_min": 32, "waves_per_cu": 0}
LOW = {"refill_min": 1, "blas_min": 1, "blas_exit": 1, "shade_min": 1, "waves_per_cu": 3}        # tests/test_gpu_parity.py SCHED_VARIANTS
HIGH = {"refill_min": 64, "blas_min": 64, "blas_exit": 64, "shade_min": 64, "waves_per_cu": 32}


def blobs(width, height, places, material=None, n_spheres=0):
    """Blobs of 24 x 20 resting on the ground at `places` (x, z, scale), C3's camera; optionally spheres."""
    b = scenes.MeshSceneBuilder()
    mat = material if material is not None else scenes._params((0.75, 0.55, 0.35), (0.15, 0.15, 0.15), (0, 0, 0), 0.55)
    for k, (x, z, s) in enumerate(places):
        v, t = scenes.uv_blob(24, 20, phase=0.7 * k)
        b.add(v, t, scenes.trs(translate=(x, -float(v[:, 1].min()) * s, z), scale=s, yaw_deg=25.0 * k), mat)
    mo, vv, ii, nn, bvh = b.finish()
    extra = {}
    if n_spheres:
        sp = scenes.make_spheres(n_spheres, 4.0, seed=0xF05E)
        extra = {"spheres": sp, "sphere_bvh": scenes.build_object_bvh(*scenes.sphere_bounds(sp))}
    return scenes.Scene(f"blobs{len(places)}", width, height, 8, 1, mesh_objects=mo, vertices=vv, indices=ii, normals=nn, mesh_bvh=bvh,
                        sky=scenes.make_sky(64, 32), **extra)


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, options, front mode) of a case.  Cached: the cases that share a scene share its oracle frames too."""
    c3 = lambda w=96, h=64: scenes.config3(w, h, slices=24, stacks=20, sky=scenes.make_sky(64, 32))
    if name in ("C3", "thresholds-low", "thresholds-high"):
        return case_scene("C3"), {"thresholds-low": LOW, "thresholds-high": HIGH}.get(name, {}), 0
    if name == "C3-scene":
        return c3(), {}, 0
    if name == "C3-spheres":
        return blobs(96, 64, [(0.0, -4.0, 2.2)], n_spheres=4), {}, 0
    if name == "mixed":
        return scenes.mixed_test_scene(96, 64), {"top_front": 0}, 0
    if name == "two-meshes":
        return blobs(96, 64, [(-2.0, -4.0, 1.6), (2.2, -2.5, 1.4)]), {"front_list": 0}, 1
    if name == "three-rays":
        sc = c3(); sc.num_rays = 3
        return sc, {}, 0
    if name == "one-bounce":
        sc = c3(); sc.num_bounces = 1
        return sc, {}, 0
    if name == "roulette":                                      # specChance + diffChance = 0.3: seven paths in ten end at their first hit of the blob
        return blobs(96, 64, [(0.0, -4.0, 2.2)], material=scenes._params((0.3, 0.1, 0.2), (0.1, 0.05, 0.1), (0.4, 0.3, 0.2), 0.5)), {}, 0
    if name in ("1x1", "65x3", "7x130"):
        w, h = (int(v) for v in name.split("x"))
        return c3(w, h), {}, 0
    raise ValueError(name)


def case_scene(name):
    return case(name + "-scene")[0]


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def differing(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).any(axis=2).sum())


def restore(ctx):
    for k, v in RESTORE.items():
        ctx.set_option(k, v)


def four_frames(ctx, sc, fuse):
    ctx.set_option("front_fuse", fuse)
    m = RayTraceMaster(ctx, sc)
    for _ in range(FRAMES):
        m.OnRenderImage()
    t, c = m._target.GetPixels(), m._converged.GetPixels()
    info = ctx.launch_info()
    tree = ctx.read_scene_blas(len(sc.mesh_objects))[:3]
    m.OnDisable()
    return t, c, info, tree


_oracle_frames = {}


def oracle_frames(sc, tree):
    """(last traced frame, accumulated image) of the FRAMES frames, once per scene object."""
    if id(sc) not in _oracle_frames:
        o = pyoracle.Oracle(sc)
        o.set_blas(*tree)
        acc, img = np.zeros((sc.height, sc.width, 4), np.float32), None
        for f in range(FRAMES):
            ox, oy, sd = scenes.frame_uniforms(f)
            o.set_frame((ox, oy), sd)
            img = o.render(mode=1, threads=8)
            acc = pyoracle.accumulate(img, acc, f)
        _oracle_frames[id(sc)] = (sc, img, acc)
    return _oracle_frames[id(sc)][1:]


@pytest.mark.parametrize("name", ["C3", "C3-spheres", "mixed", "two-meshes", "three-rays", "one-bounce", "roulette", "thresholds-low",
                                  "thresholds-high", "1x1", "65x3", "7x130"])
def test_fused_equals_voted_equals_oracle(gpu_ctx, name):
    sc, opts, front = case(name)
    try:
        for k, v in opts.items():
            gpu_ctx.set_option(k, v)
        t0, c0, i0, tree = four_frames(gpu_ctx, sc, 0)
        t1, c1, i1, _ = four_frames(gpu_ctx, sc, 1)
        ta, ca, ia, _ = four_frames(gpu_ctx, sc, -1)
        multi = "true" if sc.num_rays > 1 else "false"
        for i in (i0, i1, ia):
            assert i["n_frames"] == FRAMES and i["kernel_mode"] == 3 and i["front_mode"] == front, i
            assert i["kernel"].startswith("k_sched<false, ") and i["kernel"].endswith(f", {front}, {multi}, false>"), i
        img, acc = oracle_frames(sc, tree)
        assert same(t1, t0) and same(c1, c0), f"{name}: front_fuse 1 differs from 0 in {differing(t1, t0)} / {differing(c1, c0)} pixels"
        assert same(ta, t1) and same(ca, c1), f"{name}: front_fuse -1 differs from 1 in {differing(ta, t1)} / {differing(ca, c1)} pixels"
        assert same(t1, img) and same(c1, acc), f"{name}: front_fuse 1 differs from the oracle in {differing(t1, img)} / {differing(c1, acc)} pixels"
        assert gpu_ctx.counters()["watchdog_trips"] == 0
    finally:
        restore(gpu_ctx)


@pytest.mark.parametrize("name", ["C3", "C3-spheres", "two-meshes"])
def test_counters_equal_the_oracles_when_fused(gpu_ctx, name):
    sc, opts, front = case(name)
    try:
        for k, v in opts.items():
            gpu_ctx.set_option(k, v)
        gpu_ctx.set_option("front_fuse", 1)
        gpu_ctx.set_option("count_stats", 1)
        m = RayTraceMaster(gpu_ctx, sc)
        gpu_ctx.reset_counters()
        m.OnRenderImage()
        got = m._target.GetPixels()
        gc = gpu_ctx.counters()
        info = gpu_ctx.launch_info()
        o = pyoracle.Oracle(sc)
        o.set_blas(*gpu_ctx.read_scene_blas(len(sc.mesh_objects))[:3])
        m.OnDisable()
        assert info["count_stats"] == 1 and info["front_mode"] == front and info["kernel"].startswith("k_sched<true, "), info
        ref, oc = o.render(mode=1, threads=8, counters=True)
        assert same(got, ref)
        for k in ("rays", "tlas_nodes", "blas_nodes", "tri_tests", "sphere_tests", "hit_tri", "hit_sphere", "hit_ground", "hit_sky", "pixels"):
            assert gc[k] == oc[k], (k, gc[k], oc[k])
        assert gc["watchdog_trips"] == 0
    finally:
        restore(gpu_ctx)


def test_option_range(gpu_ctx):
    try:
        for bad in (-2, 2):
            with pytest.raises(UrtError):
                gpu_ctx.set_option("front_fuse", bad)
    finally:
        restore(gpu_ctx)
