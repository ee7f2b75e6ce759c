"""GPU: RayTraceMaster.device_object_heaps — SkinMeshes, MorphMeshes and MoveObjects with the object-level heaps built on the device
(include/urt.h "the object-level BVH on the device").  Frames after an update are held, bit for bit, to a from-scratch preparation on a
second context of the restated scene whose heaps are the host chain's, host_scene.build_object_bvh(host_scene.*_leaf_bounds(...)), and
to the oracle's literal walk; the counters that do not depend on the triangle BVHs (the updated context refits them in place, the second
one builds them anew) are equal too, and the buffer states show what crossed the bus."""
import copy

import numpy as np
import pytest

import skin_ref as S
from oracle import pyoracle
from test_gpu_deform import N_BLOB, SMALL, frame, mixed, other_ctx, restore, start, with_vertices  # noqa: F401  (other_ctx: a fixture)
from test_gpu_morph import blob_shapes, morphed_scene
from test_gpu_object_bvh import assert_nodes_equal
from test_gpu_refit import bits_equal, fresh_frame
from unityraytracer_amd import RayTraceMaster, host_scene, scenes

pytestmark = pytest.mark.gpu

F = np.float32
NB = N_BLOB[SMALL[1]]
# what a frame counts that does not depend on the shape of a triangle BVH
COUNTED = ("rays", "tlas_nodes", "sphere_tests", "hit_tri", "hit_sphere", "hit_ground", "hit_sky", "pixels", "dispatches")


def host_chain(sc):
    """The scene with the heaps every host of the library uploads today."""
    out = copy.copy(sc)
    out.mesh_bvh = host_scene.build_object_bvh(host_scene.mesh_leaf_bounds(sc.mesh_objects, sc.vertices, sc.indices))
    out.sphere_bvh = host_scene.build_object_bvh(host_scene.sphere_leaf_bounds(sc.spheres))
    return out


def device_master(ctx, sc, builder=0):
    m, _ = start(ctx, copy.copy(sc), builder)
    m.device_object_heaps = True
    return m


def four_frames(ctx, m):
    ctx.reset_counters()
    m._frame = 0; m._currentSample = 0
    for _ in range(4):
        m.OnRenderImage()
    img = m._converged.GetPixels()
    c = ctx.counters()
    return img, {k: c[k] for k in COUNTED}


def fresh_four(ctx, sc, builder=0):
    ctx.set_option("kernel_mode", 3)
    ctx.set_option("blas_builder", builder)
    m = RayTraceMaster(ctx, sc)
    out = four_frames(ctx, m)
    m.OnDisable()
    return out


def downloads(ctx, m):
    return {name: ctx.buffer_state(b)["downloads"] for name, b in (("vertices", m._vertexBuffer), ("normals", m._normalBuffer),
                                                                  ("mesh_bvh", m._meshObjectBVHBuffer), ("sphere_bvh", m._sphereBVHBuffer))}


def check_update(ctx, other, m, nxt, before, what, expect_downloads):
    """After an update of `m`: one frame and four frames against the restated scene `nxt` (heaps: the host chain's)."""
    got = frame(m)
    after = downloads(ctx, m)
    delta = {k: after[k] - before[k] for k in after}
    print(what, "downloads", delta)
    assert delta == expect_downloads, (what, delta)
    assert bits_equal(got, fresh_frame(other, nxt)), f"{what}: frame differs from a from-scratch preparation"
    assert bits_equal(got, pyoracle.Oracle(nxt).render(mode=0, threads=8)), f"{what}: frame differs from the oracle's literal walk"
    img, counted = four_frames(ctx, m)
    want_img, want_counted = fresh_four(other, nxt)
    print(what, "counters", counted, want_counted)
    assert bits_equal(img, want_img), f"{what}: four frames differ from a from-scratch preparation"
    assert counted == want_counted, (what, counted, want_counted)
    return got


def count_on(*ctxs):
    for c in ctxs:
        c.set_option("count_stats", 1)


def count_off(*ctxs):
    for c in ctxs:
        c.set_option("count_stats", 0)


ONLY_THE_HEAP = {"vertices": 0, "normals": 0, "mesh_bvh": 1, "sphere_bvh": 0}      # the preparation's own download of the small table


def test_skin_meshes_with_device_heaps(gpu_ctx, other_ctx):
    sc = mixed()
    idx, wgt, bones = S.two_bone_bend(sc.vertices[:NB], 40.0)
    try:
        count_on(gpu_ctx, other_ctx)
        m = device_master(gpu_ctx, sc)
        m.AttachSkin(0, idx, wgt)
        before = downloads(gpu_ctx, m)
        m.SkinMeshes({0: bones})
        v, n = S.skin(sc.vertices[:NB], sc.normals[:NB], idx, wgt, bones)
        vertices, normals = sc.vertices.copy(), sc.normals.copy()
        vertices[:NB], normals[:NB] = v, n
        nxt = host_chain(with_vertices(sc, vertices, normals=normals, heap=False))
        check_update(gpu_ctx, other_ctx, m, nxt, before, "SkinMeshes", ONLY_THE_HEAP)
        # the host lists are behind the device until they are asked for
        assert bits_equal(np.asarray(m.scene.vertices), sc.vertices) and m._heapsBehind == [True, False]
        m.SyncObjectHeaps()
        assert_nodes_equal(m.scene.mesh_bvh, nxt.mesh_bvh, "SyncObjectHeaps")
        assert m._heapsBehind == [False, False]                                   # (a RebuildTrees here would upload the scene's REST positions, as
        m.OnDisable()                                                             # after any SkinMeshes: test_move_objects_with_device_heaps has it)
        gpu_ctx.synchronize()
    finally:
        count_off(gpu_ctx, other_ctx)
        restore(gpu_ctx)


def test_morph_meshes_with_device_heaps(gpu_ctx, other_ctx):
    sc = mixed()
    targets = blob_shapes(sc, NB)
    w = np.array([1.0, 0.5, 1.0], F)
    try:
        count_on(gpu_ctx, other_ctx)
        m = device_master(gpu_ctx, sc)
        m.AttachBlendShapes(0, targets)
        before = downloads(gpu_ctx, m)
        m.MorphMeshes({0: w})
        nxt = host_chain(morphed_scene(sc, NB, targets, w, None))
        check_update(gpu_ctx, other_ctx, m, nxt, before, "MorphMeshes", ONLY_THE_HEAP)
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        count_off(gpu_ctx, other_ctx)
        restore(gpu_ctx)


def moved(sc, mesh_edits, sphere_edits):
    out = copy.copy(sc)
    out.mesh_objects, out.spheres = sc.mesh_objects.copy(), sc.spheres.copy()
    for k, mat in mesh_edits.items():
        out.mesh_objects[k]["localToWorldMatrix"] = mat
    for k, (pos, radius) in sphere_edits.items():
        out.spheres[k]["position"], out.spheres[k]["radius"] = pos, radius
    return host_chain(out)


EDITS = ({1: scenes.trs(translate=(2.0, 1.3, -0.5), scale=1.1, yaw_deg=15.0)}, {0: ((0.5, 1.0, 2.0), 0.75), 2: ((-1.0, 0.5, 3.0), 0.4)})


@pytest.mark.parametrize("temporal", [False, True])
def test_move_objects_with_device_heaps(gpu_ctx, other_ctx, temporal):
    sc = mixed()
    try:
        count_on(gpu_ctx, other_ctx)
        m = device_master(gpu_ctx, sc)
        if temporal:
            m.EnableTemporalAccumulation()
            for _ in range(2):
                m.OnRenderImage()
        before = downloads(gpu_ctx, m)
        m.MoveObjects(*EDITS)
        assert m._heapsBehind == [True, True]
        nxt = moved(sc, *EDITS)
        both = {"vertices": 0, "normals": 0, "mesh_bvh": 1, "sphere_bvh": 1}
        if temporal:
            m.DisableTemporalAccumulation()                                        # the frames below are compared without history
        got = check_update(gpu_ctx, other_ctx, m, nxt, before, f"MoveObjects temporal={temporal}", both)
        m.SyncObjectHeaps()
        assert_nodes_equal(m.scene.mesh_bvh, nxt.mesh_bvh, "mesh heap")
        assert_nodes_equal(m.scene.sphere_bvh, nxt.sphere_bvh, "sphere heap")
        m._heapsBehind = [True, True]                                             # RebuildTrees reads the heaps back itself before it uploads
        m.scene.mesh_bvh = m.scene.sphere_bvh = None
        m.RebuildTrees()                                                          # ... and uploads what the device holds: no pixel changes
        assert_nodes_equal(m.scene.mesh_bvh, nxt.mesh_bvh, "mesh heap after RebuildTrees")
        assert_nodes_equal(m.scene.sphere_bvh, nxt.sphere_bvh, "sphere heap after RebuildTrees")
        assert m._heapsBehind == [False, False]
        assert bits_equal(frame(m), got)
        # only one kind edited: the other heap is left alone
        before = downloads(gpu_ctx, m)
        m.MoveObjects(sphere_edits={1: ((0.0, 0.6, 1.0), 0.5)})
        assert m._heapsBehind == [False, True]
        frame(m)
        after = downloads(gpu_ctx, m)
        assert (after["mesh_bvh"] - before["mesh_bvh"], after["sphere_bvh"] - before["sphere_bvh"]) == (0, 1)
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        count_off(gpu_ctx, other_ctx)
        restore(gpu_ctx)


def test_frames_deferred_before_the_update_render_the_old_scene(gpu_ctx):
    sc = mixed()
    idx, wgt, bones = S.two_bone_bend(sc.vertices[:NB], 40.0)

    def protocol(fpl, update):
        gpu_ctx.set_option("frames_per_launch", fpl)
        m = RayTraceMaster(gpu_ctx, copy.copy(sc))
        m.device_object_heaps = True
        m.AttachSkin(0, idx, wgt)
        m.OnRenderImage()                                                         # (the buffers exist from here on)
        old = None
        for _ in range(3):
            m.OnRenderImage()                                                     # dispatched before the update: the old scene
        if update:
            converged = m._converged                                              # (SkinMeshes restarts the accumulation; the image stays)
            m.SkinMeshes({0: bones})
            old = converged.GetPixels()
            m.OnRenderImage()
            new = m._target.GetPixels()
        else:
            old, new = m._converged.GetPixels(), None
        m.OnDisable()
        return old, new

    try:
        batched_old, batched_new = protocol(4, True)
        immediate_old, immediate_new = protocol(1, True)
        plain_old, _ = protocol(4, False)
        assert bits_equal(batched_old, immediate_old) and bits_equal(batched_old, plain_old)
        assert bits_equal(batched_new, immediate_new) and not bits_equal(batched_new, plain_old)
    finally:
        restore(gpu_ctx)


def test_flag_off_is_the_host_path(gpu_ctx, other_ctx):
    sc = mixed()
    idx, wgt, bones = S.two_bone_bend(sc.vertices[:NB], 40.0)
    try:
        other_ctx.set_option("refit", 1)
        a, _ = start(gpu_ctx, copy.copy(sc), 0)
        a.device_object_heaps = False
        b, _ = start(other_ctx, copy.copy(sc), 0)                                 # a master that never heard of the attribute
        frames = []
        for m in (a, b):
            m.AttachSkin(0, idx, wgt)
            m.SkinMeshes({0: bones})
            frames.append([frame(m)])
            m.MoveObjects(*EDITS)
            frames[-1].append(frame(m))
            assert list(m._leafBuffers) == [None, None] and list(m._heapsBehind) == [False, False]
        assert bits_equal(frames[0][0], frames[1][0]) and bits_equal(frames[0][1], frames[1][1])
        assert downloads(gpu_ctx, a)["mesh_bvh"] == 0 and downloads(gpu_ctx, a)["sphere_bvh"] == 0      # the host uploaded its heaps
        for node_a, node_b in ((a.scene.mesh_bvh, b.scene.mesh_bvh), (a.scene.sphere_bvh, b.scene.sphere_bvh)):
            assert node_a.tobytes() == node_b.tobytes()
        a.OnDisable(); b.OnDisable()
        gpu_ctx.synchronize()
    finally:
        other_ctx.set_option("refit", 0)
        restore(gpu_ctx)
        restore(other_ctx)
        other_ctx.set_option("refit", 0)
