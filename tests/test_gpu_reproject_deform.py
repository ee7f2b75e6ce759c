"""GPU: temporal reprojection with per-vertex motion (include/urt.h urt_reproject_deformed, urt_buffer_copy; RayTraceMaster.DeformMeshes /
SkinMeshes with keep_history) — bit for bit against the float32 restatement of tests/reproject_deform_ref.py on random images and random
previous-position buffers that hit every dead case, and on real renders whose meshes were deformed through DeformMeshes and SkinMeshes;
the equivalences with urt_reproject_objects; the device-side snapshot; errors, counters and deferred frames; and the quality on the
pixels of a deforming mesh against today's default and a fresh frame."""
import copy
import ctypes as C

import numpy as np
import pytest

import reproject_deform_cases as K
import skin_ref as S
from reproject_deform_ref import (QUALITY_BLOB, QUALITY_CAMERA, QUALITY_MESH, QUALITY_MIN_COVERAGE, QUALITY_MIN_KEPT, QUALITY_PHASE, QUALITY_SIZE,
                                  matrices_of, reproject_deformed_ref)
from reproject_motion_ref import IDENTITY, reproject_objects_ref
from unityraytracer_amd import Context, RayTraceMaster, _lib, host_scene, scenes
from unityraytracer_amd.unity_api import ComputeBuffer, ComputeShader, RenderTexture

pytestmark = pytest.mark.gpu

F = np.float32


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits(got, ref, what):
    g, r = u32(got), u32(ref)
    bad = g != r
    assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} texels differ, first at {np.argwhere(bad)[0]}: {got[tuple(np.argwhere(bad)[0][:2])]} " \
                          f"vs {ref[tuple(np.argwhere(bad)[0][:2])]}"


def assert_outputs(got, ref, what, motion=True):
    for key in ("color", "count") + (("motion",) if motion else ()):
        assert_bits(got[key], ref[key], f"{what} {key}")


def library_deform(deform):
    """The deform tuple of the cases (matrices as (n, 16)) as reproject_arrays takes it (records of 112 bytes)."""
    return (deform[0], deform[1], K.mesh_object_records(deform[2]), deform[3]) + tuple(deform[4:])


# ---- 1. random inputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", K.SIZES)
def test_random_inputs_match_reference_bit_for_bit(gpu_ctx, size):
    w, h = size
    kept = with_history = dead = 0
    for k in range(len(K.SETTINGS)):                       # with and without tables, with and without a motion image
        images, mats, params, motion = K.settings_case(k, 1000 * w + 10 * h + k, w, h, move=k != 3)
        ref = reproject_deformed_ref(*images, *mats, **params)
        deform = params.pop("deform")
        got = gpu_ctx.reproject_arrays(*images, *mats, motion=motion, deform=library_deform(deform), **params)
        assert_outputs(got, ref, f"{w}x{h} case {k}", motion)
        kept += int(ref["kept"].sum())
        with_history += int((ref["count"][..., 0][ref["kept"]] > 0).sum())
        dead += int((ref["deformed"] & ~ref["kept"]).sum())
    if w * h > 1000:                                       # the cases do exercise the per-vertex path, with and without history, and its dead ends
        assert kept > 0.01 * w * h and with_history > 20 and dead > 0.01 * w * h, (kept, with_history, dead)


# ---- 2. the equivalences ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(17, 33), (96, 64)])
def test_zero_flags_and_null_deform_equal_reproject_objects_bit_for_bit(gpu_ctx, size):
    w, h = size
    images, mats, params, _ = K.settings_case(0, 7 * w, w, h)
    deform = params.pop("deform")
    objects = gpu_ctx.reproject_arrays(*images, *mats, **params)
    assert_outputs(objects, reproject_objects_ref(*images, *mats, **params), "objects")
    zero = (deform[0], deform[1], deform[2], np.zeros_like(deform[3]), deform[4])
    got = gpu_ctx.reproject_arrays(*images, *mats, deform=library_deform(zero), **params)
    o, kind = images[7].view(np.int32)[..., 0], images[6][..., 3]
    inside = ~((kind == 3) & ((o < 0) | (o >= len(deform[3]))))                  # a triangle pixel outside the tables has no history by definition
    for key in ("color", "count", "motion"):
        assert u32(got[key])[inside].tobytes() == u32(objects[key])[inside].tobytes(), key
        assert (got[key][~inside] == 0).all(), key
    assert inside.mean() > 0.7
    # urt_reproject_deformed itself with deform == NULL, with and without motion
    with Context(gpu_ctx.device) as ctx:
        tex = [RenderTexture(ctx, w, h) for _ in range(11)]
        for t, a in zip(tex, images):
            t.SetPixels(a)
        sh = ComputeShader(ctx)
        sh.SetMatrix("_CameraToWorld", mats[1])
        sh.SetMatrix("_CameraInverseProjection", mats[2])
        tabs = [ComputeBuffer(ctx, len(params[n]), 48) for n in ("mesh_motion", "sphere_motion")]
        for b, n in zip(tabs, ("mesh_motion", "sphere_motion")):
            b.SetData(params[n])
        im = _lib.ReprojectImages(*(t.handle for t in tex))
        p = _lib.ReprojectParams((C.c_float * 16)(*mats[0].tolist()), params["max_history"], params["normal_threshold"], params["plane_threshold"], 0)
        mo = _lib.ReprojectMotion(tabs[0].handle, tabs[1].handle, params["moved_max_history"], 0)
        plain = reproject_objects_ref(*images, *mats, max_history=params["max_history"], normal_threshold=params["normal_threshold"],
                                      plane_threshold=params["plane_threshold"])
        for motion, want in ((C.byref(mo), objects), (None, plain)):
            for t in tex[8:]:
                t.SetPixels(np.full((h, w, 4), 7.0, F))
            assert ctx.lib.urt_reproject_deformed(ctx._h, C.byref(im), C.byref(p), motion, None) == 0
            for t, key in zip(tex[8:], ("color", "count", "motion")):
                assert_bits(t.GetPixels(), want[key], f"NULL deform {key}")
        for t in tex + tabs:
            t.Release()


# ---- 3. real renders -------------------------------------------------------------------------------------------------------------------
SMALL = ((96, 64), (12, 9))
N_BLOB = 12 * 8 + 2


def near_scene(size=SMALL[0], blob=SMALL[1], position=(-1.0, 1.5, -4.0)):
    sc = scenes.mixed_test_scene(*size, blob=blob)
    sc.camera_to_world, sc.camera_inverse_projection = scenes.camera_matrices(*size, position=position)   # the default camera sees the blob 8 pixels tall
    return sc


def started(ctx, sc, frames=6, **temporal):
    m = RayTraceMaster(ctx, sc)
    m.EnableTemporalAccumulation(**temporal)
    for _ in range(frames):
        m.OnRenderImage()
    return m


def check_step(m, sc, step, edited, what, threshold=_lib.REPROJECT_DEFORM_NORMAL_THRESHOLD):
    """One keep_history step: the history before it, the call, then colour, count and motion against the restatement fed with the
    library's own feature buffers and its own previous-positions buffer."""
    ctx = m.ctx
    hist_color, hist_count = m._converged.GetPixels(), m._tcount.GetPixels()
    prev_mo = sc.mesh_objects.copy()
    cam = (sc.camera_to_world.copy(), sc.camera_inverse_projection.copy())
    step()
    prev = [t.GetPixels() for t in m._taov[0]]
    cur = [t.GetPixels() for t in m._taov[1]]
    extra = [RenderTexture(ctx, m.screen_width, m.screen_height) for _ in range(3)]   # the motion image: the same call once more (the spare pair holds the old history)
    ctx.reproject(m._tspare[0], m._tspare[1], *m._taov[0], *m._taov[1], extra[0], extra[1], scenes.world_to_clip(*cam), motion=extra[2],
                  mesh_motion=m._tmotion[0], moved_max_history=m._moved_max_history, deform=m._deform_argument(edited), **m._temporal)
    motion = extra[2].GetPixels()
    assert extra[0].GetPixels().tobytes() == m._converged.GetPixels().tobytes() and extra[1].GetPixels().tobytes() == m._tcount.GetPixels().tobytes()
    for t in extra:
        t.Release()
    prev_v = m._tdeform[0].GetData().view(F).reshape(-1, 3)
    flags = np.zeros(len(prev_mo), np.int32)
    flags[list(edited)] = 1
    table = host_scene.mesh_motion(prev_mo, prev_mo)
    ref = reproject_deformed_ref(hist_color, hist_count, *prev, *cur, scenes.world_to_clip(*cam), *cam, mesh_motion=table,
                                 moved_max_history=m._moved_max_history, deform=(prev_v, sc.indices, matrices_of(prev_mo), flags, threshold), **m._temporal)
    assert_bits(m._converged.GetPixels(), ref["color"], what + " color")
    assert_bits(m._tcount.GetPixels(), ref["count"], what + " count")
    assert_bits(motion, ref["motion"], what + " motion")
    return ref, prev_v, cur


def test_deform_meshes_keeps_the_history_and_matches_the_reference(gpu_ctx):
    sc = near_scene()
    v_new = scenes.uv_blob(12, 9, phase=0.5)[0]
    with Context(gpu_ctx.device) as ctx:
        m = started(ctx, copy.copy(sc), moved_max_history=16.0)
        before = np.array(m.scene.vertices, F)
        ref, prev_v, cur = check_step(m, m.scene, lambda: m.DeformMeshes({0: v_new}, keep_history=True), [0], "DeformMeshes")
        assert prev_v.tobytes() == before.tobytes()                             # the snapshot holds the positions the history saw
        on = (cur[2].view(np.int32)[..., 0] == 0) & (cur[1][..., 3] == 3)
        assert on.mean() > 0.02 and (ref["deformed"] == on).all()
        kept = ref["count"][..., 0][on] > 0
        assert kept.mean() >= 0.5, kept.mean()
        assert ref["count"][..., 0][on].max() <= 16.0                           # moved_max_history clamps deformed pixels as it clamps moved ones
        assert np.abs(ref["motion"][..., :2][on]).max() > 0.05                  # and the motion image holds the surface's own motion
        assert (ref["count"][..., 0][~on] > 0).mean() >= 0.9
        assert ctx.deform_stats()["deformed"] >= 1
        for _ in range(2):
            m.OnRenderImage()
        # a second step from the deformed state, with another threshold
        m._deform_normal_threshold = 0.8
        v2 = scenes.uv_blob(12, 9, phase=0.9)[0]
        check_step(m, m.scene, lambda: m.DeformMeshes({0: v2}, recompute_normals=False, keep_history=True), [0], "second step", threshold=0.8)
        m.OnDisable()


def test_skin_meshes_keeps_the_history_without_a_download(gpu_ctx):
    sc = near_scene()
    with Context(gpu_ctx.device) as ctx:
        m = started(ctx, copy.copy(sc))
        idx, wgt, bones = S.two_bone_bend(sc.vertices[:N_BLOB], 12.0)
        m.AttachSkin(0, idx, wgt)
        m.SkinMeshes({0: bones}, keep_history=True)
        for _ in range(2):
            m.OnRenderImage()
        assert ctx.buffer_state(m._vertexBuffer)["downloads"] == 0 and ctx.buffer_state(m._tdeform[0])["downloads"] == 0
        state = ctx.buffer_state(m._tdeform[0])
        assert (state["stale_first"], state["stale_last"]) == (0, len(sc.vertices) - 1) and state["mirror_bytes"] == 12 * len(sc.vertices)
        first_pose = S.skin(sc.vertices[:N_BLOB], sc.normals[:N_BLOB], idx, wgt, bones)[0]
        # the second pose starts from device-written positions: the snapshot copies them where they are
        bones2 = S.two_bone_bend(sc.vertices[:N_BLOB], 20.0)[2]
        vb, pb = m._vertexBuffer, None

        def step():
            m.SkinMeshes({0: bones2}, keep_history=True)
            nonlocal pb
            pb = m._tdeform[0]
            assert ctx.buffer_state(vb)["downloads"] == 0 and ctx.buffer_state(pb)["downloads"] == 0   # before the check reads them back
        ref, prev_v, cur = check_step(m, m.scene, step, [0], "SkinMeshes")
        assert prev_v[:N_BLOB].tobytes() == np.ascontiguousarray(first_pose, F).tobytes() and prev_v[N_BLOB:].tobytes() == sc.vertices[N_BLOB:].tobytes()
        on = (cur[2].view(np.int32)[..., 0] == 0) & (cur[1][..., 3] == 3)
        assert on.mean() > 0.02 and (ref["count"][..., 0][on] > 0).mean() >= 0.5
        assert ctx.buffer_state(vb)["downloads"] == 0                           # (the check read the snapshot, not the vertex buffer)
        m.OnDisable()


def test_keep_history_false_is_what_it_was(gpu_ctx):
    """DeformMeshes / SkinMeshes without keep_history, with it False, and with it True while temporal accumulation is off."""
    sc = near_scene()
    v_new = scenes.uv_blob(12, 9, phase=0.5)[0]
    idx, wgt, bones = S.two_bone_bend(sc.vertices[:N_BLOB], 12.0)
    out = []
    for variant in ("default", "false"):
        with Context(gpu_ctx.device) as ctx:
            m = started(ctx, copy.copy(sc))
            kw = {} if variant == "default" else {"keep_history": False}
            m.DeformMeshes({0: v_new}, **kw)
            a = (m._converged.GetPixels(), m._tcount.GetPixels())
            m.OnRenderImage()
            m.AttachSkin(0, idx, wgt)
            m.SkinMeshes({0: bones}, **kw)
            out.append(a + (m._converged.GetPixels(), m._tcount.GetPixels()))
            assert m._tdeform == [None, None, None]
            on = (m._taov[1][2].GetPixels().view(np.int32)[..., 0] == 0) & (m._taov[1][1].GetPixels()[..., 3] == 3)
            assert on.any() and (out[-1][3][..., 0][on] == 0).all()              # the pinned default: no history on a deformed mesh
            m.OnDisable()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
    with Context(gpu_ctx.device) as ctx:                                        # temporal accumulation off: keep_history changes nothing
        m = RayTraceMaster(ctx, copy.copy(sc))
        for _ in range(2):
            m.OnRenderImage()
        m.DeformMeshes({0: v_new}, keep_history=True)
        assert m._currentSample == 0 and m._tdeform == [None, None, None]
        m.OnDisable()


# ---- 4. eight small meshes ---------------------------------------------------------------------------------------------------------------
def test_every_other_of_eight_meshes_is_deformed(gpu_ctx):
    sc = scenes.many_meshes_scene(96, 64, n=8, level=1)
    sc.camera_to_world, sc.camera_inverse_projection = scenes.camera_matrices(96, 64, position=(-0.6, 1.2, -0.5), pitch_deg=10.0)
    with Context(gpu_ctx.device) as ctx:
        m = started(ctx, sc)
        rng = np.random.default_rng(8)
        edits = {}
        for k in range(0, 8, 2):
            lo, hi = m.vertex_span(k)
            v = np.array(sc.vertices[lo: hi + 1], F)
            edits[k] = (v * (1.0 + 0.06 * rng.standard_normal((len(v), 1)))).astype(F)   # every vertex moves along its radius
        hist_color, hist_count = m._converged.GetPixels(), m._tcount.GetPixels()
        ref, _, cur = check_step(m, sc, lambda: m.DeformMeshes(edits, keep_history=True), list(edits), "eight meshes")
        o, kind = cur[2].view(np.int32)[..., 0], cur[1][..., 3]
        even = (kind == 3) & (o % 2 == 0)
        assert even.sum() > 50 and (kind == 3).sum() - even.sum() > 50
        assert (ref["deformed"] == even).all()
        # only the deformed meshes lose their urt_reproject_objects behaviour
        cam = (sc.camera_to_world, sc.camera_inverse_projection)
        objects = reproject_objects_ref(hist_color, hist_count, *[t.GetPixels() for t in m._taov[0]], *cur, scenes.world_to_clip(*cam), *cam,
                                        mesh_motion=np.tile(IDENTITY, (8, 1)), **m._temporal)
        for key in ("color", "count"):
            assert u32(ref[key])[~even].tobytes() == u32(objects[key])[~even].tobytes(), key
        assert (ref["count"][..., 0][even] > 0).mean() > 0.5
        m.OnDisable()


# ---- 5. urt_buffer_copy ------------------------------------------------------------------------------------------------------------------
def test_buffer_copy(gpu_ctx):
    rng = np.random.default_rng(11)
    with Context(gpu_ctx.device) as ctx:
        a, b = ComputeBuffer(ctx, 100, 12), ComputeBuffer(ctx, 160, 12)
        da = rng.normal(size=(100, 3)).astype(F)
        db = rng.normal(size=(160, 3)).astype(F)
        a.SetData(da)
        b.SetData(db)
        assert ctx.buffer_state(a)["mirror_bytes"] == 0
        b.CopyFrom(a, 0, 0, 10)                                                 # both ends of both buffers
        b.CopyFrom(a, 90, 150, 10)
        sa, sb = ctx.buffer_state(a), ctx.buffer_state(b)
        assert sa["mirror_bytes"] == 1200 and sb["mirror_bytes"] == 1920 and sa["downloads"] == sb["downloads"] == 0
        assert (sa["stale_first"], sa["stale_last"]) == (1, 0)                   # the source is only read
        assert (sb["stale_first"], sb["stale_last"]) == (0, 159)                 # one range, as with SetDataDevice
        want = db.copy()
        want[:10], want[150:] = da[:10], da[90:]
        assert b.GetData().view(F).reshape(-1, 3).tobytes() == want.tobytes()
        assert ctx.buffer_state(b)["downloads"] == 1 and ctx.buffer_state(a)["downloads"] == 0
        # a source written on the device is copied from where it was written; a host SetData after the copy does not reach the snapshot
        c = ComputeBuffer(ctx, 100, 12)
        c.CopyFrom(a)
        a.SetData(da + 1)
        d = ComputeBuffer(ctx, 100, 12)
        d.CopyFrom(c, 5, 5, 90)
        got = d.GetData().view(F).reshape(-1, 3)
        assert got[5:95].tobytes() == da[5:95].tobytes() and (got[:5] == 0).all() and (got[95:] == 0).all()
        assert ctx.buffer_state(c)["downloads"] == 0 and ctx.buffer_state(a)["downloads"] == 0
        assert a.GetData().view(F).reshape(-1, 3).tobytes() == (da + 1).tobytes()
        d.CopyFrom(a, 0, 0, 0)                                                  # count 0: nothing
        # errors enqueue nothing and mark nothing
        e, wide = ComputeBuffer(ctx, 50, 12), ComputeBuffer(ctx, 50, 16)
        lib, hd = ctx.lib, ctx._h
        cases = [((0, 0, e.handle, 0, 1), 2), ((a.handle, 0, 0, 0, 1), 2), ((987654, 0, e.handle, 0, 1), 2), ((a.handle, 0, 987654, 0, 1), 2),
                 ((a.handle, 0, wide.handle, 0, 1), 1), ((a.handle, -1, e.handle, 0, 1), 1), ((a.handle, 0, e.handle, -1, 1), 1),
                 ((a.handle, 0, e.handle, 0, -1), 1), ((a.handle, 95, e.handle, 0, 6), 1), ((a.handle, 0, e.handle, 45, 6), 1),
                 ((a.handle, 0, e.handle, 0, 51), 1), ((e.handle, 0, e.handle, 10, 5), 1), ((a.handle, 2 ** 31 - 1, e.handle, 0, 2 ** 31 - 1), 1)]
        for args, code in cases:
            assert lib.urt_buffer_copy(hd, *args) == code, (args, code)
        se = ctx.buffer_state(e)
        assert se["mirror_bytes"] == 0 and (se["stale_first"], se["stale_last"]) == (1, 0) and (e.GetData() == 0).all()
        for x in (a, b, c, d, e, wide):
            x.Release()


# ---- 6. errors; no side effects ---------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(gpu_ctx):
    w, h = 16, 8
    rng = np.random.default_rng(6)
    with Context(gpu_ctx.device) as ctx:
        lib, hd = ctx.lib, ctx._h
        names = ("prev_color", "prev_count", "prev_hit", "prev_normal", "prev_id", "hit", "normal", "id", "color", "count", "motion")
        tex = {n: RenderTexture(ctx, w, h) for n in names}
        snap = {}
        for n, t in tex.items():
            a = rng.uniform(-2, 2, (h, w, 4)).astype(F)
            t.SetPixels(a)
            snap[n] = a
        pv, ix, mo_, fl = ComputeBuffer(ctx, 9, 12), ComputeBuffer(ctx, 6, 4), ComputeBuffer(ctx, 3, 112), ComputeBuffer(ctx, 3, 4)
        ix4, fl4, table = ComputeBuffer(ctx, 4, 4), ComputeBuffer(ctx, 4, 4), ComputeBuffer(ctx, 3, 48)
        table.SetData(np.tile(IDENTITY, (3, 1)))
        gone = ComputeBuffer(ctx, 4, 4)
        gone_h = gone.handle
        gone.Release()
        im = C.byref(_lib.ReprojectImages(*(tex[n].handle for n in names)))
        M = (C.c_float * 16)(*np.eye(4, dtype=F).reshape(16).tolist())
        p = C.byref(_lib.ReprojectParams(M, 64.0, 0.9, 0.02, 0))
        mo = C.byref(_lib.ReprojectMotion(table.handle, 0, 0.0, 0))

        def de(v=pv.handle, i=ix.handle, o=mo_.handle, f=fl.handle, nt=0.5, flags=0):
            return C.byref(_lib.ReprojectDeform(v, i, o, f, nt, flags))
        assert lib.urt_reproject_deformed(hd, im, p, mo, de()) == 5                     # URT_ERR_UNBOUND: no camera matrices yet
        sh = ComputeShader(ctx)
        sh.SetMatrix("_CameraToWorld", scenes.camera_matrices(w, h)[0])
        sh.SetMatrix("_CameraInverseProjection", scenes.camera_matrices(w, h)[1])
        cases = [((None, p, mo, de()), 1), ((im, None, mo, de()), 1),
                 ((im, p, mo, de(v=0)), 2), ((im, p, mo, de(i=0)), 2), ((im, p, mo, de(o=0)), 2), ((im, p, mo, de(f=0)), 2),
                 ((im, p, mo, de(v=987654)), 2), ((im, p, mo, de(f=gone_h)), 2), ((im, p, mo, de(i=tex["hit"].handle)), 2),
                 ((im, p, mo, de(v=ix.handle)), 1), ((im, p, mo, de(i=pv.handle)), 1), ((im, p, mo, de(o=table.handle)), 1), ((im, p, mo, de(f=mo_.handle)), 1),
                 ((im, p, mo, de(i=ix4.handle)), 1),                                      # four indices: no multiple of 3
                 ((im, p, mo, de(f=fl4.handle)), 1),                                      # four flags for three MeshObjects
                 ((im, p, mo, de(flags=1)), 1), ((im, p, mo, de(nt=float("nan"))), 1),
                 ((im, p, C.byref(_lib.ReprojectMotion(table.handle, 0, 0.5, 0)), de()), 1),
                 ((im, C.byref(_lib.ReprojectParams(M, 64.0, float("nan"), 0.02, 0)), mo, de()), 1),
                 ((C.byref(_lib.ReprojectImages(*([tex["hit"].handle] * 11))), p, mo, de()), 1)]
        for k, (args, code) in enumerate(cases):
            assert lib.urt_reproject_deformed(hd, *args) == code, (k, code)
        for n, t in tex.items():
            assert t.GetPixels().tobytes() == snap[n].tobytes(), n
        assert lib.urt_reproject_deformed(hd, im, p, mo, de()) == 0                      # and a valid call does write
        assert lib.urt_reproject_deformed(hd, im, p, None, de(nt=float("inf"))) == 0
        assert tex["color"].GetPixels().tobytes() != snap["color"].tobytes()
        for b in (pv, ix, mo_, fl):
            assert ctx.buffer_state(b)["downloads"] == 0 and ctx.buffer_state(b)["mirror_bytes"] > 0
        for t in list(tex.values()) + [pv, ix, mo_, fl, ix4, fl4, table]:
            t.Release()


def test_counters_unrelated_textures_and_deferred_frames(gpu_ctx):
    sc = near_scene((48, 32))
    with Context(gpu_ctx.device) as ctx:
        ctx.set_option("count_stats", 1)
        m = started(ctx, sc)
        bystander = RenderTexture(ctx, 48, 32)
        marks = np.random.default_rng(5).uniform(0, 1, (32, 48, 4)).astype(F)
        bystander.SetPixels(marks)
        prev, cur = m._taov
        ctx.render_aov(prev[0], prev[1], None, prev[2])
        ctx.render_aov(cur[0], cur[1], None, cur[2])
        ctx.synchronize()
        for _ in range(4):
            m.OnRenderImage()                                                      # deferred: _converged is a pending blend's destination
        pv = np.array(sc.vertices, F)
        pv[:N_BLOB] *= F(1.02)
        bufs = [ComputeBuffer(ctx, len(pv), 12), ComputeBuffer(ctx, len(sc.mesh_objects), 112), ComputeBuffer(ctx, len(sc.mesh_objects), 4)]
        flags = np.array([1, 0, 0], np.int32)
        for b, a in zip(bufs, (pv, sc.mesh_objects, flags)):
            b.SetData(a)
        c0 = ctx.counters()
        spare = RenderTexture(ctx, 48, 32)
        M = scenes.world_to_clip(sc.camera_to_world, sc.camera_inverse_projection)
        ctx.reproject(m._converged, m._tcount, *prev, *cur, m._tspare[0], m._tspare[1], M, motion=spare,
                      deform=(bufs[0], m._indexBuffer, bufs[1], bufs[2]))
        got = (m._tspare[0].GetPixels(), m._tspare[1].GetPixels(), spare.GetPixels())
        assert ctx.counters() == c0
        assert bystander.GetPixels().tobytes() == marks.tobytes()
        conv, cnt = m._converged.GetPixels(), m._tcount.GetPixels()
        assert (cnt[..., 0] == 10).all()                                          # all ten frames were in the history the call saw
        ref = reproject_deformed_ref(conv, cnt, *[x.GetPixels() for x in prev], *[x.GetPixels() for x in cur], M, sc.camera_to_world,
                                     sc.camera_inverse_projection, deform=(pv, sc.indices, matrices_of(sc.mesh_objects), flags))
        for g, key in zip(got, ("color", "count", "motion")):
            assert_bits(g, ref[key], "deferred " + key)
        assert ref["kept"].any()
        for b in bufs + [m._indexBuffer]:
            assert ctx.buffer_state(b)["downloads"] == 0
        for x in [bystander, spare] + bufs:
            x.Release()
        m.OnDisable()


# ---- 7. quality ---------------------------------------------------------------------------------------------------------------------------
def quality_scene(phase):
    w, h = QUALITY_SIZE
    sc = scenes.mixed_test_scene(w, h, blob=QUALITY_BLOB)
    sc.camera_to_world, sc.camera_inverse_projection = scenes.camera_matrices(w, h, position=QUALITY_CAMERA)
    v = np.array(sc.vertices, F)
    v[: len(scenes.uv_blob(*QUALITY_BLOB)[0])] = scenes.uv_blob(*QUALITY_BLOB, phase=phase)[0]
    sc.vertices = v
    sc.normals = host_scene.compute_normals(sc.vertices, sc.indices)
    sc.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(sc.mesh_objects, sc.vertices, sc.indices))
    return sc


def quality(ctx, frames=64, ref_frames=1024, thresholds=(None,)):
    """MSE against a ref_frames accumulation of the deformed scene, on the pixels of the deformed mesh: (A) DeformMeshes with
    keep_history (one entry per threshold), (B) today's default, each followed by one frame; (C) a fresh one-frame image; and the share of
    those pixels that have history after the call in A and in B."""
    new_v = scenes.uv_blob(*QUALITY_BLOB, phase=QUALITY_PHASE[1])[0]
    runs = {}
    for variant in [("A", t) for t in thresholds] + [("B", None)]:
        m = started(ctx, quality_scene(QUALITY_PHASE[0]), frames, deform_normal_threshold=variant[1])
        m.DeformMeshes({QUALITY_MESH: new_v}, keep_history=variant[0] == "A")
        count = m._tcount.GetPixels()[..., 0]
        normal, ids = m._taov[1][1].GetPixels(), m._taov[1][2].GetPixels()
        m.OnRenderImage()
        runs[variant] = (m._converged.GetPixels()[..., :3].astype(np.float64), count)
        m.OnDisable()
    mask = (normal[..., 3] == 3) & (ids.view(np.int32)[..., 0] == QUALITY_MESH)
    deformed = quality_scene(QUALITY_PHASE[1])
    ref_m = RayTraceMaster(ctx, deformed, frame_seed=0xBEEF)
    for _ in range(ref_frames):
        ref_m.OnRenderImage()
    ref = ref_m._converged.GetPixels()[..., :3].astype(np.float64)
    ref_m.OnDisable()
    fresh_m = RayTraceMaster(ctx, deformed, frame_seed=0x0F1E)
    fresh_m.OnRenderImage()
    fresh = fresh_m._converged.GetPixels()[..., :3].astype(np.float64)
    fresh_m.OnDisable()
    mse = lambda a: float(((a - ref)[mask] ** 2).mean())  # noqa: E731
    out = dict(mse_b=mse(runs[("B", None)][0]), mse_c=mse(fresh), share_b=float((runs[("B", None)][1][mask] > 0).mean()), coverage=float(mask.mean()))
    out["a"] = {t: (mse(runs[("A", t)][0]), float((runs[("A", t)][1][mask] > 0).mean())) for t in thresholds}
    out["mse_a"], out["share_a"] = out["a"][thresholds[0]]
    return out


# Measured on one MI355X (DESIGN.md "Per-vertex motion", profiles/r18_logs/quality_thresholds.log): the deformed blob covers 14.1 % of the
# image; with the default threshold (0.3) 99.9 % of its pixels keep history in A and none in B; MSE A 7.47e-3, B 7.99e-1, C (a fresh
# frame) 7.15e-1: C/A = 96x, B/A = 107x.  The floor is under half of the measured C/A, the margin tests/test_gpu_reproject.py and
# tests/test_gpu_reproject_motion.py took, to ride out seed-to-seed noise.
QUALITY_FLOOR = 40.0


def test_quality_on_the_deformed_mesh(gpu_ctx):
    with Context(gpu_ctx.device) as ctx:
        q = quality(ctx)
    print(f"deformed-mesh quality: coverage {q['coverage']:.3f}; pixels with history A {q['share_a']:.3f}, B {q['share_b']:.3f}; "
          f"MSE A {q['mse_a']:.4e}, B {q['mse_b']:.4e}, C {q['mse_c']:.4e}; C/A {q['mse_c'] / q['mse_a']:.1f}x, B/A {q['mse_b'] / q['mse_a']:.1f}x")
    assert q["coverage"] >= QUALITY_MIN_COVERAGE, q
    assert q["share_a"] >= QUALITY_MIN_KEPT and q["share_b"] == 0, q
    assert q["mse_a"] < q["mse_b"] and q["mse_a"] < q["mse_c"], q
    assert q["mse_c"] >= QUALITY_FLOOR * q["mse_a"], q
