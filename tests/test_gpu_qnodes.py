"""GPU: the quantized triangle-BVH nodes of option "qnodes" (csrc/qnodes.hip k_qframe / k_quantize, the QN loop of k_sched).
- the nodes the library derives equal their restatement (tests/qnodes_ref.py) bit for bit, on trees of every builder;
- with qnodes = 1 every frame equals the qnodes = 0 frame and the oracle's (mode 1 on the product's own tree) bit for bit, and runs one of
  the 16 k_sched<false, B, F, M, true> instantiations; all 16 are seen;
- the auto mode, refits that grow and shrink the grid, and switching the option between frames.
Quantized boxes only cull (conservatively), so pixels must not change; tests/test_qnodes_ref.py checks the margins that make it so."""
import copy

import numpy as np
import pytest

import qnodes_ref as Q
from oracle import pyoracle
from test_gpu_fuzz import random_scene
from test_gpu_refit import moved_scene, reupload
from test_qnodes_ref import MARGIN_TOL, margins
from unityraytracer_amd import Context, RayTraceMaster, UrtError, scenes

pytestmark = pytest.mark.gpu

RESTORE = {"qnodes": 0, "count_stats": 0, "kernel_mode": 3, "blas_builder": -1, "sched_block": 0, "top_nodes": -1, "top_front": -1,
           "front_list": -1, "refit": 1}


def restore(ctx):
    for k, v in RESTORE.items():
        ctx.set_option(k, v)


def render(ctx, sc, qn, frames=1, m=None):
    """(target, converged, kernel name) of `frames` frames of kernel mode 3 with option qnodes = qn (None: as it is — setting the option
    prepares the scene from scratch)."""
    if qn is not None:
        ctx.set_option("qnodes", qn)
    ctx.set_option("count_stats", 0)
    ctx.set_option("kernel_mode", 3)
    own = m is None
    if own:
        m = RayTraceMaster(ctx, sc)
    for _ in range(frames):
        m.OnRenderImage()
    t, c = m._target.GetPixels(), m._converged.GetPixels()
    kernel = ctx.launch_info()["kernel"]
    if own:
        m.OnDisable()
    return t, c, kernel


def oracle_frames(ctx, sc, frames):
    """The oracle's mode 1 on the product's tree (read back from the bound scene): (last target, converged)."""
    o = pyoracle.Oracle(sc)
    if len(sc.mesh_objects):
        nodes, tri, root, _ = ctx.read_scene_blas(len(sc.mesh_objects))
        o.set_blas(nodes, tri, root)
    acc = np.zeros((sc.height, sc.width, 4), np.float32)
    img = None
    for i in range(frames):
        ox, oy, sd = scenes.frame_uniforms(i)
        o.set_frame((ox, oy), sd)
        img = o.render(mode=1 if len(sc.mesh_objects) else 0, threads=8)
        acc = pyoracle.accumulate(img, acc, i)
    return img, acc


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_readback(ctx, sc, option=1, expect_in_use=True):
    """The bound scene's quantized nodes equal the restatement of its float nodes, bit for bit, and keep their margins; the traversal
    reads them exactly when the restatement of the host's rule says so."""
    nodes, _, root, _ = ctx.read_scene_blas(len(sc.mesh_objects))
    frame, words, in_use = ctx.read_scene_qnodes()
    rf, rw = Q.quantized_nodes(nodes, root)
    assert same(frame, rf), (sc.name, frame, rf)
    assert np.array_equal(words, rw), (sc.name, int((words != rw).any(axis=1).sum()), len(rw))
    assert in_use == Q.in_use(rf, option) == expect_in_use, (sc.name, in_use)
    ml, mh = margins(nodes, frame, words)
    assert ml.min() >= 2 - MARGIN_TOL and mh.min() >= 2 - MARGIN_TOL, (sc.name, ml.min(), mh.min())
    return frame


def frame_check(ctx, sc, frames=1, what=""):
    """qnodes = 1 == qnodes = 0 == oracle, bit for bit; the QN loop ran.  -> the QN kernel's name."""
    t0, c0, k0 = render(ctx, sc, 0, frames)
    assert k0.endswith(", false>"), k0
    m = RayTraceMaster(ctx, sc)
    t1, c1, k1 = render(ctx, sc, 1, frames, m)
    ref_t, ref_c = oracle_frames(ctx, sc, frames)
    m.OnDisable()
    ctx.synchronize()
    assert k1.endswith(", true>"), (what, k1)
    assert same(t1, t0) and same(c1, c0), f"{what}: qnodes 1 differs from qnodes 0 in {int((t1.view(np.uint32) != t0.view(np.uint32)).any(axis=2).sum())} pixels"
    assert same(t1, ref_t) and same(c1, ref_c), f"{what}: qnodes 1 differs from the oracle in {int((t1.view(np.uint32) != ref_t.view(np.uint32)).any(axis=2).sum())} pixels"
    assert ctx.counters()["watchdog_trips"] == 0
    return k1


EDGE = [k for k in scenes.QNODE_EDGE_KINDS]


@pytest.mark.parametrize("builder", [0, 1, 2, 3])
def test_readback_equals_the_restatement(gpu_ctx, builder):
    try:
        gpu_ctx.set_option("blas_builder", builder)
        gpu_ctx.set_option("qnodes", 1)
        for sc in [scenes.mixed_test_scene(64, 40, blob=(40, 31)), scenes.many_meshes_scene(64, 40), scenes.deep_chain_scene(64, 40)] + \
                  [scenes.qnode_edge_scene(k, 33, 21) for k in EDGE]:
            m = RayTraceMaster(gpu_ctx, sc)
            m.OnRenderImage()
            check_readback(gpu_ctx, sc, 1, sc.name != "deep-chain")
            m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        restore(gpu_ctx)


def test_readback_is_empty_while_the_option_is_off(gpu_ctx):
    sc = scenes.mixed_test_scene(32, 20)
    restore(gpu_ctx)
    m = RayTraceMaster(gpu_ctx, sc)
    m.OnRenderImage()
    frame, words, in_use = gpu_ctx.read_scene_qnodes()
    m.OnDisable()
    assert len(words) == 0 and not in_use


@pytest.mark.parametrize("seed", range(8))
def test_fuzz_scenes_bit_exact(gpu_ctx, seed):
    s = 5000 + seed
    sc, _, frames = random_scene(s)
    while not len(sc.mesh_objects):                                # (a scene without MeshObjects has no triangle BVH to quantize)
        s += 100
        sc, _, frames = random_scene(s)
    try:
        gpu_ctx.set_option("blas_builder", seed % 4)                # the host builder and the three GPU builders take turns
        frame_check(gpu_ctx, sc, frames, sc.name)
    finally:
        restore(gpu_ctx)


@pytest.mark.parametrize("name", ["mixed", "many_meshes"] + EDGE)
@pytest.mark.parametrize("top", [-1, 0])
def test_scenes_bit_exact(gpu_ctx, name, top):
    sc = {"mixed": lambda: scenes.mixed_test_scene(120, 72, blob=(40, 31)), "many_meshes": lambda: scenes.many_meshes_scene(96, 60)}.get(
        name, lambda: scenes.qnode_edge_scene(name))()
    try:
        gpu_ctx.set_option("top_nodes", top)
        frame_check(gpu_ctx, sc, 2, f"{name} top_nodes {top}")
    finally:
        restore(gpu_ctx)


def test_all_sixteen_instantiations(gpu_ctx):
    """k_sched<false, B, F, M, true>: B = sched_block 64 / 256; F = front mode 0 (one MeshObject), 1 (front_list 0), 2 (front_list 2),
    3 (the masked default of a multi-mesh scene); M = numRays > 1."""
    single = scenes.qnode_edge_scene("floor", 40, 24)
    single.mesh_objects = single.mesh_objects[:1]
    single.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(single.mesh_objects, single.vertices, single.indices))
    multi = scenes.mixed_test_scene(40, 24, blob=(40, 31))
    seen = set()
    try:
        for block in (64, 256):
            for fmode, sc0, opts in ((0, single, {}), (1, multi, {"front_list": 0}), (2, multi, {"front_list": 2}), (3, multi, {})):
                for rays in (1, 2):
                    sc = copy.copy(sc0)
                    sc.num_rays = rays
                    restore(gpu_ctx)
                    gpu_ctx.set_option("sched_block", block)
                    for k, v in opts.items():
                        gpu_ctx.set_option(k, v)
                    k = frame_check(gpu_ctx, sc, 1, f"block {block} front {fmode} rays {rays}")
                    want = f"k_sched<false, {block}, {fmode}, {'true' if rays > 1 else 'false'}, true>"
                    assert k == want, (k, want)
                    seen.add(k)
    finally:
        restore(gpu_ctx)
    assert len(seen) == 16


def tiny_beside_large():
    b = scenes.MeshSceneBuilder()
    v, t = scenes.icosphere(1)
    b.add(v, t, scenes.trs(translate=(0, 1, 0), scale=0.002), scenes._params((0.8, 0.3, 0.2), (0.1, 0.1, 0.1), (0, 0, 0), 0.5))
    b.add(*scenes.grid_quad((-300, 0.2, -300), (600, 0, 0), (0, 0, 600), 4, (0, -1, 0)), scenes.trs(), scenes._params((0.6, 0.6, 0.6), (0.1, 0.1, 0.1), (0, 0, 0), 0.3))
    mo, vv, ii, nn, bvh = b.finish()
    sc = scenes.Scene("tiny-beside-large", 64, 40, 3, 1, mesh_objects=mo, vertices=vv, indices=ii, normals=nn, mesh_bvh=bvh, sky=scenes.make_sky(64, 32))
    return sc.resized(64, 40, position=(0.0, 1.0, -0.012), fov_deg=30.0)


def test_auto_and_forcing(gpu_ctx):
    tiny = tiny_beside_large()
    compact = scenes.mixed_test_scene(64, 40, blob=(40, 31))
    try:
        gpu_ctx.set_option("qnodes", -1)
        for sc, want in ((tiny, False), (compact, True)):
            m = RayTraceMaster(gpu_ctx, sc)
            _, _, k = render(gpu_ctx, sc, -1, 1, m)
            frame = check_readback(gpu_ctx, sc, -1, want)
            m.OnDisable()
            assert k.endswith(", true>" if want else ", false>"), (sc.name, k, frame[0, 3])
            assert (frame[0, 3] >= 1024) == want
        frame_check(gpu_ctx, tiny, 2, "tiny mesh, qnodes 1")            # forced: still bit-exact, no watchdog
        gpu_ctx.synchronize()
    finally:
        restore(gpu_ctx)


@pytest.fixture(scope="module")
def other_ctx():
    ctx = Context(0)
    ctx.set_option("refit", 0)
    yield ctx
    ctx.close()


def test_refit_keeps_the_nodes_exact(gpu_ctx, other_ctx):
    """Rigid moves, a non-uniform scale, and a MeshObject moved outside the old grid (the frame grows) and back (it shrinks)."""
    sc = scenes.mixed_test_scene(96, 60, blob=(40, 31))
    steps = [
        {1: scenes.trs(translate=(2.7, 1.2, -0.6), yaw_deg=10.0)},
        {0: scenes.trs(translate=(-1.2, 1.6, 0.4), scale=(2.1, 0.45, 1.3), yaw_deg=-71.0)},
        {1: scenes.trs(translate=(40.0, 25.0, 60.0), scale=3.0)},
        {1: scenes.trs(translate=(2.5, 1.0, -1.0), yaw_deg=-20.0)},
    ]
    try:
        gpu_ctx.set_option("qnodes", 1)
        other_ctx.set_option("qnodes", 1)
        m = RayTraceMaster(gpu_ctx, sc)
        render(gpu_ctx, sc, None, 1, m)
        r0, _ = gpu_ctx.refit_stats()
        cur, cells = sc, []
        for edits in steps:
            cur = moved_scene(cur, edits)
            reupload(m, cur)
            t1, c1, k = render(gpu_ctx, cur, None, 1, m)
            assert k.endswith(", true>"), k
            cells.append(check_readback(gpu_ctx, cur)[1, :3].copy())
            ref_t, _ = oracle_frames(gpu_ctx, cur, 1)
            assert same(t1, ref_t), "refitted frame differs from the oracle"
            ft, _, fk = render(other_ctx, cur, 1, 1)
            assert fk.endswith(", true>") and same(t1, ft), "refitted frame differs from a from-scratch preparation"
        assert gpu_ctx.refit_stats()[0] > r0
        assert (cells[2] > cells[1]).any() and (cells[3] < cells[2]).any()       # the grid grew, then shrank
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        other_ctx.set_option("qnodes", 0)
        restore(gpu_ctx)


def test_switching_the_option_between_frames(gpu_ctx):
    sc = scenes.qnode_edge_scene("floor", 64, 40)
    try:
        m = RayTraceMaster(gpu_ctx, sc)
        got = []
        for qn in (0, 1, 0):
            m._frame = 0; m._currentSample = 0
            t, _, k = render(gpu_ctx, sc, qn, 1, m)
            assert k.endswith(", true>" if qn else ", false>"), (qn, k)
            got.append(t)
        ref_t, _ = oracle_frames(gpu_ctx, sc, 1)
        m.OnDisable()
        for t in got:
            assert same(t, ref_t)
        for bad in (-2, 2):
            with pytest.raises(UrtError) as e:
                gpu_ctx.set_option("qnodes", bad)
            assert e.value.code == 1, e.value                     # URT_ERR_INVALID_ARGUMENT
    finally:
        restore(gpu_ctx)
