"""GPU: the normal cones of option "blas_cones" (csrc/cones.hip, the cone test of k_sched in csrc/trace_device.h).
1. The words read back from the device meet the obligation of tests/cones_ref.py on the triangle records they were derived from — also
   after a refit that turns the MeshObject by 90 degrees about x (the words change with the normals).
2. Frames of 96 x 64, four frames in one launch, kernel mode 3: blas_cones 1 == blas_cones 0 == the oracle, bit for bit — reduced C3, C4
   (masked FRONT, and the top walk inside the plain FRONT) and C5 (listed FRONT), a flat grid seen edge-on from just above and just below
   its plane, two layers of opposite windings, and the deep chain.
3. With count_stats the counters equal the oracle's: the counting instantiation walks without cones."""

import numpy as np
import pytest

import cones_ref as K
from oracle import pyoracle
from test_gpu_refit import moved_scene, reupload
from unityraytracer_amd import RayTraceMaster, scenes

pytestmark = pytest.mark.gpu

RESTORE = {"blas_cones": -1, "count_stats": 0, "kernel_mode": 3, "front_list": -1, "blas_builder": -1, "refit": 1}
FRAMES = 4


def restore(ctx):
    for k, v in RESTORE.items():
        ctx.set_option(k, v)


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def random_directions(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def rot_x90(translate, scale):
    """localToWorldMatrix (16 floats, column-major): scale, then a quarter turn about x, then the translation."""
    m = np.eye(4)
    m[:3, :3] = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]) * scale
    m[:3, 3] = translate
    return np.ascontiguousarray(m.T.astype(np.float32).reshape(16))


def device_cones(ctx, sc):
    """(words, first, count, e1, e2) of the bound scene: the device's words and records, the ranges of the device's tree."""
    nodes, _, root, _ = ctx.read_scene_blas(len(sc.mesh_objects))
    words, e1, e2, in_use = ctx.read_scene_cones()
    assert in_use and len(words) == len(nodes)
    first, count = K.child_ranges(nodes, root)
    return words, first, count, e1, e2


@pytest.mark.parametrize("kind", K.CONE_MESHES)
def test_device_words_meet_the_obligation_before_and_after_a_refit(gpu_ctx, kind):
    sc = K.cone_scene(kind, 32, 24)
    common = random_directions(2000, 11)
    try:
        gpu_ctx.set_option("blas_cones", 1)
        m = RayTraceMaster(gpu_ctx, sc)
        m.OnRenderImage()
        w0, first, count, e1, e2 = device_cones(gpu_ctx, sc)
        n_skips, n_cones = K.check_obligation(w0, first, count, e1, e2, common)
        assert n_cones > 0 and n_skips > 1000, (n_cones, n_skips)
        if kind == "blob":
            leaf = np.ascontiguousarray(gpu_ctx.read_scene_blas(1)[0][:, 12:14]).view(np.int32) < 0
            assert K.own_axis_skips(w0)[leaf].mean() >= 0.5
        r0, _ = gpu_ctx.refit_stats()
        turned = moved_scene(sc, {0: rot_x90((0.0, 1.6, -5.0), 1.3)})
        reupload(m, turned)
        m.OnRenderImage()
        assert gpu_ctx.refit_stats()[0] == r0 + 1                        # refitted, not rebuilt
        w1, first1, count1, f1, f2 = device_cones(gpu_ctx, turned)
        assert np.array_equal(first, first1) and np.array_equal(count, count1)
        assert not np.array_equal(f1, e1) and (w1 != w0).any(), "the cones did not follow the refitted triangles"
        n_skips, n_cones = K.check_obligation(w1, first1, count1, f1, f2, common)
        assert n_cones > 0 and n_skips > 1000, (n_cones, n_skips)
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        restore(gpu_ctx)


def test_words_are_zero_while_the_option_is_off(gpu_ctx):
    sc = K.cone_scene("blob", 32, 24)
    try:
        gpu_ctx.set_option("blas_cones", 0)
        m = RayTraceMaster(gpu_ctx, sc)
        m.OnRenderImage()
        words, _, _, in_use = gpu_ctx.read_scene_cones()
        info = gpu_ctx.launch_info()
        m.OnDisable()
        assert not in_use and len(words) > 0 and not words.any() and info["cones"] == 0
    finally:
        restore(gpu_ctx)


def edge_on(dy):
    """The flat grid (facing up, plane y = 1) from a level camera dy above its plane: the primaries sweep through d . n = 0."""
    sc = K.cone_scene("grid", 96, 64, matrix=scenes.trs(translate=(0.0, 1.0, -5.0), scale=1.5))
    return sc.resized(96, 64, position=(0.0, 1.0 + dy, -10.0), fov_deg=40.0)


def reduced(name):
    sky = scenes.make_sky(64, 32)
    if name == "C3":
        return scenes.config3(96, 64, slices=40, stacks=31, sky=sky), {}, 0
    if name == "C4":
        return scenes.config4(96, 64, slices=24, stacks=21, sky=sky), {}, 3
    if name == "C4-plain-front":
        return scenes.config4(96, 64, slices=24, stacks=21, sky=sky), {"front_list": 0}, 1
    if name == "C5-listed":
        return scenes.config5(96, 64, level=2, n_blobs=12, sky=sky), {"front_list": 2}, 2
    if name == "C5":
        return scenes.config5(96, 64, level=2, n_blobs=12, sky=sky), {}, 3
    if name == "grid-above":
        return edge_on(3e-4), {}, 0
    if name == "grid-below":
        return edge_on(-3e-4), {}, 0
    if name == "pair":
        return K.cone_scene("pair"), {}, 0
    if name == "deep-chain":
        return scenes.deep_chain_scene(96, 64), {}, 0
    raise ValueError(name)


def four_frames(ctx, sc, cones):
    ctx.set_option("blas_cones", cones)
    m = RayTraceMaster(ctx, sc)
    for _ in range(FRAMES):
        m.OnRenderImage()
    t, c = m._target.GetPixels(), m._converged.GetPixels()
    info = ctx.launch_info()
    nodes, tri, root, _ = ctx.read_scene_blas(len(sc.mesh_objects))
    words = ctx.read_scene_cones()[0]
    m.OnDisable()
    return t, c, info, (nodes, tri, root), words


@pytest.mark.parametrize("name", ["C3", "C4", "C4-plain-front", "C5", "C5-listed", "grid-above", "grid-below", "pair", "deep-chain"])
def test_frames_bit_exact(gpu_ctx, name):
    sc, opts, front = reduced(name)
    sc.num_bounces = min(sc.num_bounces, 8)
    try:
        for k, v in opts.items():
            gpu_ctx.set_option(k, v)
        t0, c0, i0, tree, w_off = four_frames(gpu_ctx, sc, 0)
        t1, c1, i1, _, w_on = four_frames(gpu_ctx, sc, 1)
        assert i0["cones"] == 0 and i1["cones"] == 1 and not w_off.any() and w_on.any(), (i0, i1)
        for i in (i0, i1):
            assert i["n_frames"] == FRAMES and i["kernel_mode"] == 3 and i["front_mode"] == front and i["kernel"].endswith(", false, false>"), i
        o = pyoracle.Oracle(sc)
        o.set_blas(*tree)
        acc, img = np.zeros((sc.height, sc.width, 4), np.float32), None
        for f in range(FRAMES):
            ox, oy, sd = scenes.frame_uniforms(f)
            o.set_frame((ox, oy), sd)
            img = o.render(mode=1, threads=8)
            acc = pyoracle.accumulate(img, acc, f)
        diff = lambda a, b: int((a.view(np.uint32) != b.view(np.uint32)).any(axis=2).sum())
        assert same(t1, t0) and same(c1, c0), f"{name}: blas_cones 1 differs from 0 in {diff(t1, t0)} / {diff(c1, c0)} pixels"
        assert same(t1, img) and same(c1, acc), f"{name}: blas_cones 1 differs from the oracle in {diff(t1, img)} / {diff(c1, acc)} pixels"
        assert gpu_ctx.counters()["watchdog_trips"] == 0
    finally:
        restore(gpu_ctx)


@pytest.mark.parametrize("name", ["C3", "C4"])
def test_counters_equal_the_oracles_with_cones_on(gpu_ctx, name):
    sc, _, _ = reduced(name)
    sc.num_bounces = 4
    try:
        gpu_ctx.set_option("blas_cones", 1)
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
        assert info["count_stats"] == 1 and info["cones"] == 0 and info["kernel"].startswith("k_sched<true, "), info
        ref, oc = o.render(mode=1, threads=8, counters=True)
        assert same(got, ref)
        for k in ("rays", "tlas_nodes", "blas_nodes", "tri_tests", "hit_tri", "hit_ground", "hit_sky", "pixels"):
            assert gc[k] == oc[k], (k, gc[k], oc[k])
    finally:
        restore(gpu_ctx)
