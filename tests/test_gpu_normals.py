"""GPU: the normals on the device (include/urt.h urt_normals_plan_create / urt_compute_normals; csrc/normals.hip over the plan of
csrc/normals_plan.cpp) and RayTraceMaster.RecomputeNormals / SkinMeshes(recompute_normals=True) on top of them.  The kernels are held
to the numpy restatement of tests/normals_ref.py and to host_scene.compute_normals bit for bit (a NaN equals a NaN: the host's and the
device's default NaN differ); frames after a device-side deformation are held, bit for bit, to a from-scratch preparation on a second
context of those positions with the host's normals and to the oracle's literal walk, and the counters show that neither positions nor
normals touched the host."""
import copy
import ctypes as C

import numpy as np
import pytest

import normals_ref as N
import skin_ref as S
from test_gpu_deform import DEEP, N_BLOB, SMALL, frame, mixed, other_ctx, restore, start, stats, with_vertices  # noqa: F401  (other_ctx: a fixture)
from test_gpu_refit import bits_equal, fresh_frame
from test_gpu_skin import check_skinned_frame, f32, same
from unityraytracer_amd import ComputeBuffer, Context, RayTraceMaster, RayTraceObject, _lib, host_scene, live_resources, scenes

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = F(7.5)
INVALID_ARGUMENT, INVALID_HANDLE, SCENE = 1, 2, 8


class Raw:
    """A vertices and an indices buffer holding (v, t), and a destination of the vertex count filled with a sentinel."""

    def __init__(self, ctx, v, t):
        self.ctx, self.v, self.t = ctx, np.ascontiguousarray(v, F), np.ascontiguousarray(t, np.int32)
        self.V, self.I, self.D = ComputeBuffer(ctx, len(self.v), 12), ComputeBuffer(ctx, len(self.t), 4), ComputeBuffer(ctx, len(self.v), 12)
        self.V.SetData(self.v)
        self.I.SetData(self.t)
        self.reset()

    def reset(self):
        self.D.SetData(np.full((len(self.v), 3), SENTINEL, F))

    def all(self):
        return (self.V, self.I, self.D)

    def release(self):
        for b in self.all():
            b.Release()


def check_plan(ctx, raw, first, count, what, positions=None):
    """One plan over raw's buffers, computed once for the buffer's positions and once per entry of `positions` (host SetData of the
    vertices, which the mirror follows) — always against the restatement with the plan of the FIRST positions."""
    want_plan = N.plan(raw.v, raw.t, first, count)
    plan = ctx.normals_plan(raw.V, raw.I, first, count)
    info = plan.info
    nt, ne = len(want_plan["tris"]), len(want_plan["entries"])
    assert info == {"first": first, "count": count, "n_lists": want_plan["n_lists"], "n_triangles": nt, "n_entries": ne,
                    "max_valence": want_plan["max_valence"], "device_bytes": 4 * (3 * nt + ne + 2 * count)}, (what, info)
    inside = slice(first, first + count)
    outside = np.ones(len(raw.v), bool); outside[inside] = False
    for step, v in enumerate([raw.v] + list(positions or [])):
        if step:
            raw.V.SetData(v)
        raw.reset()
        downloads = ctx.buffer_state(raw.V)["downloads"]
        plan.compute(raw.D)
        st = ctx.buffer_state(raw.D)
        assert (st["stale_first"], st["stale_last"], st["mirror_bytes"]) == (first, first + count - 1, len(raw.v) * 12), (what, step, st)
        assert ctx.buffer_state(raw.V)["downloads"] == downloads, (what, step)
        got = f32(raw.D)
        assert same(got[inside], N.apply(want_plan, v)), (what, step)
        if N.welds_alike(raw.v, v, raw.t):
            with np.errstate(all="ignore"):
                assert same(got[inside], host_scene.compute_normals(v, raw.t)[inside]), (what, step)
        assert (got[outside] == SENTINEL).all(), (what, step)
    plan.Release()
    if positions:
        raw.V.SetData(raw.v)


# ---- 1. the kernels against the restatement ---------------------------------------------------------------------------------------------
def padded_blob(count, first):
    """The smallest of the two blobs that holds `count` vertices, behind `first` padding vertices and in front of three more."""
    size = (12, 9) if count <= N_BLOB[(12, 9)] else (40, 31)
    v, t = scenes.uv_blob(*size)
    pad = np.array([[50.0 + k, -3.0, 0.5 * k] for k in range(first + 3)], F)
    return np.concatenate([pad[:first], v, pad[first:]]), t.reshape(-1).astype(np.int32) + first


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, 1202])
def test_compute_normals_equals_the_restatement(gpu_ctx, count, first):
    v, t = padded_blob(count, first)
    assert len(v) > first + count
    raw = Raw(gpu_ctx, v, t)
    moved = [N.wobble(v, 0.7), N.wobble(v, 2.1, 0.2)]
    check_plan(gpu_ctx, raw, first, count, ("blob", first, count), positions=moved)
    raw.release()


def non_finite():
    v, t = scenes.uv_blob(12, 9)
    v = v.copy()
    v[3, 1] = np.nan; v[17] = np.nan; v[40, 0] = np.inf; v[41, 2] = -np.inf; v[90] = np.inf
    return v, t.reshape(-1).astype(np.int32)


def pole70():
    v, t = scenes.uv_blob(70, 3)                             # a pole of valence 70: one lane loops past a wave's width
    return v, t.reshape(-1).astype(np.int32)


VARIANTS = {"cube24": N.cube24, "seam_sphere": N.seam_sphere, "pole70": pole70, "odd_ones": N.odd_ones, "non_finite": non_finite,
            "partner": N.partner_case, "two_quads": N.two_quads}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variants_equal_the_restatement(gpu_ctx, name):
    v, t = VARIANTS[name]()
    if name == "pole70":
        assert N.plan(v, t)["max_valence"] == 70
    raw = Raw(gpu_ctx, v, t)
    moved = [N.wobble(v, 1.3)] if name not in ("partner", "non_finite") else None      # (a wobble would move the tiny coordinates apart)
    check_plan(gpu_ctx, raw, 0, len(v), (name, "whole"), positions=moved)
    if len(v) > 8:
        check_plan(gpu_ctx, raw, 5, len(v) - 8, (name, "span"))
    check_plan(gpu_ctx, raw, len(v) - 1, 1, (name, "last"))
    raw.release()


# ---- 2. frames --------------------------------------------------------------------------------------------------------------------------
# The mixed scene has a cross-mesh weld of its own: the blob's poles sit at (0, +-1, 0) in object space, where the icosphere holds a
# vertex too, and ComputeNormals welds across meshes.  So the deformations below leave the poles where they are (else the weld would
# split), and the icosphere's normals are recomputed with the blob's: its pole vertices take the blob's faces.
@pytest.mark.parametrize("size,builder", [(SMALL, b) for b in (0, 1, 3)] + [(DEEP, b) for b in (0, 1, 3)])
def test_frames_after_a_device_side_deformation(gpu_ctx, other_ctx, size, builder):
    import torch
    sc = mixed(size)
    nb, nv = N_BLOB[size[1]], len(sc.vertices)
    try:
        m, (nodes, tri, root) = start(gpu_ctx, copy.copy(sc), builder, 2)
        plan = gpu_ctx.normals_plan(m._vertexBuffer, m._indexBuffer)              # everything, from the rest positions; nothing is stale: no download
        assert plan.info["max_valence"] == N.plan(sc.vertices, sc.indices)["max_valence"] > size[1][0]      # (the pole and the icosphere's vertex)
        for step, phase in enumerate((0.4, 1.9, 3.3)):                            # three successive deformations, one plan
            vertices = sc.vertices.copy()
            vertices[:nb] = N.wobble(sc.vertices[:nb], phase, pin_poles=True)
            assert N.welds_alike(sc.vertices, vertices, sc.indices)               # a condition on the inputs
            d0, (r0, p0), built0 = stats(gpu_ctx)
            moved = torch.from_numpy(vertices[:nb]).to(f"cuda:{gpu_ctx.device}")   # (kept until the frame below has been waited for)
            m._vertexBuffer.SetDataDevice(moved, 0, nb)
            plan.compute(m._normalBuffer)
            lo3, hi3, n = gpu_ctx.buffer_bounds(m._vertexBuffer, 0, nb)
            assert n == nb
            m._skinBoxes[0] = (lo3, hi3)                                          # the object heap from the GPU's bounds, as SkinMeshes makes it
            m.scene.mesh_bvh = m._object_heap_with_skins()
            m._meshObjectBVHBuffer = m.CreateComputeBuffer(m._meshObjectBVHBuffer, m.scene.mesh_bvh, m.BVHNodeSize)
            nxt = with_vertices(sc, vertices, normals=host_scene.compute_normals(vertices, sc.indices), heap=False)
            assert not same(nxt.normals[nb:], sc.normals[nb:])                    # the neighbour's normals change with the blob's faces
            nxt.mesh_bvh = m.scene.mesh_bvh
            nodes = check_skinned_frame(gpu_ctx, other_ctx, m, builder, sc, nxt, nodes, tri, root, f"{size} builder {builder} step {step}",
                                        oracle=step == 0)
            d1, (r1, p1), built1 = stats(gpu_ctx)
            assert (d1["deformed"] - d0["deformed"], d1["renormed"] - d0["renormed"], r1 - r0, p1 - p0) == (1, 3, 1, 1), (d0, d1)     # in place
            assert d1["bytes_copied"] - d0["bytes_copied"] == (nb + nv) * 12 and d1["forced_rebuilds"] == d0["forced_rebuilds"]
            for buf, last in ((m._vertexBuffer, nb - 1), (m._normalBuffer, nv - 1)):      # neither positions nor normals touched the host
                st = gpu_ctx.buffer_state(buf)
                assert st["downloads"] == 0 and (st["stale_first"], st["stale_last"]) == (0, last), st
        plan.Release()
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        restore(gpu_ctx)


# ---- 3. the cross-mesh weld -------------------------------------------------------------------------------------------------------------
def test_a_plan_for_one_mesh_welds_against_its_neighbour(gpu_ctx):
    v, t = N.two_quads()
    raw = Raw(gpu_ctx, v, t)
    plan = gpu_ctx.normals_plan(raw.V, raw.I, 0, 4)                               # mesh 0's span only
    assert plan.info["n_triangles"] == 4 and plan.info["n_lists"] == 4            # the neighbour's two triangles are needed
    plan.compute(raw.D)
    got, want = f32(raw.D), host_scene.compute_normals(v, t)
    assert same(got[:4], want[:4]) and (got[4:] == SENTINEL).all()
    alone = host_scene.compute_normals(v[:4], t[:6])                              # what the mesh alone would give along the shared edge
    assert not same(want[1:3], alone[1:3])
    plan.Release(); raw.release()


# ---- 4. RayTraceMaster ------------------------------------------------------------------------------------------------------------------
def twist(vertices, angle_deg):
    """A skin that leaves the poles (0, +-1, 0) exactly where they are (their weight for the moving bone is 0, a term that is not live):
    bone 0 the identity, bone 1 a rotation about the y axis and a shift, weighted by 1 - y^2.  Blended, so not rigid."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    s = np.clip(F(1.0) - v[:, 1] * v[:, 1], F(0.0), F(1.0)).astype(F)
    idx = np.zeros((len(v), 4), np.int32)
    idx[:, 1] = 1
    wgt = np.zeros((len(v), 4), F)
    wgt[:, 0], wgt[:, 1] = F(1.0) - s, s
    c, sn = np.cos(np.radians(angle_deg)), np.sin(np.radians(angle_deg))
    R = np.array([[c, 0.0, sn], [0.0, 1.0, 0.0], [-sn, 0.0, c]])
    bones = np.zeros((2, 12), F)
    bones[0] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    bones[1] = np.concatenate([R.T.reshape(-1), [0.3, 0.0, 0.0]]).astype(F)
    return idx, wgt, bones


def posed_scene(sc, nb, idx, wgt, bones, heap, recompute):
    """The scene skinned by the restatement, with host_scene.compute_normals of the skinned positions — in the skinned span only when
    `recompute`, else the bones' normals there."""
    v, n = S.skin(sc.vertices[:nb], sc.normals[:nb], idx, wgt, bones)
    vertices = sc.vertices.copy()
    vertices[:nb] = v
    normals = host_scene.compute_normals(vertices, sc.indices)
    if not recompute:
        normals[:nb] = n
    out = with_vertices(sc, vertices, normals=normals, heap=False)
    out.mesh_bvh = heap
    return out


@pytest.mark.parametrize("builder", [0, 3])
def test_skin_meshes_with_recomputed_normals(gpu_ctx, other_ctx, builder):
    sc = mixed(SMALL)
    nb = N_BLOB[SMALL[1]]
    try:
        m, (nodes, tri, root) = start(gpu_ctx, copy.copy(sc), builder, 2)
        idx, wgt, _ = twist(sc.vertices[:nb], 40.0)
        m.AttachSkin(0, idx, wgt)
        first_pose = None
        for step, angle in enumerate((40.0, -25.0)):
            bones = twist(sc.vertices[:nb], angle)[2]
            m.SkinMeshes({0: bones}, recompute_normals=True)
            assert sorted(m._normalsPlans) == ([0] if step == 0 else [0, 1]) and m._normalsPlans[0][1].info["count"] == nb      # the skinned span only
            m.RecomputeNormals([1])                                               # the icosphere holds a vertex at each of the blob's poles (above)
            nxt = posed_scene(sc, nb, idx, wgt, bones, m.scene.mesh_bvh, True)
            first_pose = nxt.vertices if first_pose is None else first_pose
            assert N.welds_alike(first_pose, nxt.vertices, sc.indices)            # the plans of the first pose serve the second
            nodes = check_skinned_frame(gpu_ctx, other_ctx, m, builder, sc, nxt, nodes, tri, root, f"builder {builder} step {step}", oracle=step == 0)
            bones_only = posed_scene(sc, nb, idx, wgt, bones, m.scene.mesh_bvh, False)
            assert not same(bones_only.normals[:nb], nxt.normals[:nb])            # the twist is not rigid: the bones' normals are others
            got = frame(m)
            m.SkinMeshes({0: bones})
            assert not bits_equal(frame(m), got)                                  # ... and the switch does something
            assert bits_equal(frame(m), fresh_frame(other_ctx, bones_only, builder))
        assert gpu_ctx.buffer_state(m._vertexBuffer)["downloads"] == 1            # the first plan's creation from the first pose; nothing after it
        assert gpu_ctx.buffer_state(m._normalBuffer)["downloads"] == 0
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        restore(gpu_ctx)


def test_recompute_normals_makes_new_plans_after_a_lists_rebuild(gpu_ctx):
    ref = mixed(SMALL)
    try:
        m = RayTraceMaster(gpu_ctx, scenes.Scene("objs", ref.width, ref.height, 4, 1, sky=ref.sky))
        for mo in ref.mesh_objects:
            sl = ref.indices[int(mo["indices_offset"]): int(mo["indices_offset"]) + int(mo["indices_count"])]
            L = mo["lighting"]
            m.RegisterObject(RayTraceObject(type=0, vertices=ref.vertices[sl.min(): sl.max() + 1], triangles=(sl - sl.min()).reshape(-1, 3),
                                            localToWorldMatrix=mo["localToWorldMatrix"], albedoColor=tuple(L["color_albedo"]),
                                            specularColor=tuple(L["color_specular"]), emissionColor=tuple(L["emission"]), smoothness=float(L["smoothness"])))
        m.OnRenderImage()
        m._normalBuffer.SetData(np.full((len(ref.vertices), 3), SENTINEL, F))
        m.RecomputeNormals()
        assert same(f32(m._normalBuffer), m.scene.normals) and sorted(m._normalsPlans) == [0, 1, 2]
        old = {k: hit[1] for k, hit in m._normalsPlans.items()}
        handles = [p.handle for p in old.values()]
        m.RecomputeNormals([1])
        assert all(m._normalsPlans[k][1] is old[k] for k in old)                  # cached
        m.RebuildObjectLists()
        assert m._normalsPlans == {} and all(p.handle == 0 for p in old.values())      # every plan was released, the unnamed mesh's too
        info = _lib.NormalsPlanInfo()
        assert all(gpu_ctx.lib.urt_normals_plan_info(gpu_ctx._h, h, C.byref(info)) == INVALID_HANDLE for h in handles)
        m.RebuildTrees()
        m._normalBuffer.SetData(np.full((len(ref.vertices), 3), SENTINEL, F))
        m.RecomputeNormals([0, 2])
        assert sorted(m._normalsPlans) == [0, 2] and all(m._normalsPlans[k][1] is not old[k] for k in (0, 2))      # new plans
        got = f32(m._normalBuffer)
        assert same(got[:98], m.scene.normals[:98]) and (got[98:140] == SENTINEL).all() and same(got[140:], m.scene.normals[140:])
        for bad in ("0", 0.0, True):
            with pytest.raises(TypeError):
                m.RecomputeNormals([bad])
        with pytest.raises(IndexError):
            m.RecomputeNormals([3])
        m.OnDisable()
        assert m._normalsPlans == {}
        gpu_ctx.synchronize()
    finally:
        restore(gpu_ctx)


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_everything_untouched(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx._h
    v, t = N.seam_sphere()
    raw = Raw(gpu_ctx, v, t)
    n = len(v)
    plan = gpu_ctx.normals_plan(raw.V, raw.I, 2, 10)
    plan.compute(raw.D)                                                           # (a stale range to keep)
    empty = gpu_ctx.normals_plan(raw.V, raw.I, 4, 0)
    other12, other16, bad_idx, odd_idx = ComputeBuffer(gpu_ctx, n + 1, 12), ComputeBuffer(gpu_ctx, n, 16), ComputeBuffer(gpu_ctx, 6, 4), ComputeBuffer(gpu_ctx, 7, 4)
    bad_idx.SetData(np.array([0, 1, 2, 3, n, 4], np.int32))
    involved = raw.all() + (other12, other16, bad_idx, odd_idx)
    before = [gpu_ctx.buffer_state(b) for b in involved]
    d0, live0 = gpu_ctx.deform_stats(), live_resources()
    plan_info = (plan.info, empty.info)
    out = C.c_uint64(77)

    def refused(rc, code, what=None):
        """The call failed with `code` and left no trace: the state of every buffer involved, the scene's counters, the live resources
        and the plans are what they were.  Asserted after EACH call."""
        assert rc == code, (what, rc)
        assert [gpu_ctx.buffer_state(b) for b in involved] == before, what
        assert gpu_ctx.deform_stats() == d0 and live_resources() == live0 and (plan.info, empty.info) == plan_info, what

    def create(code, vertices=raw.V.handle, indices=raw.I.handle, first=0, count=5, null_out=False):
        out.value = 77
        refused(lib.urt_normals_plan_create(h, vertices, indices, first, count, None if null_out else C.byref(out)), code,
                (vertices, indices, first, count, null_out))
        assert out.value == 0 or null_out                                         # no handle comes back

    for key in ("vertices", "indices"):
        create(INVALID_HANDLE, **{key: 0})
        create(INVALID_HANDLE, **{key: 0xdead})
    create(INVALID_HANDLE, vertices=plan.handle)                                  # a plan is not a buffer
    create(INVALID_ARGUMENT, null_out=True)
    create(INVALID_ARGUMENT, vertices=other16.handle)                             # strides
    create(INVALID_ARGUMENT, indices=raw.V.handle)
    create(INVALID_ARGUMENT, indices=odd_idx.handle)                              # not triangles
    for first, count in ((-1, 1), (0, -1), (n - 3, 4), (n, 1), (2 ** 31 - 1, 2)):
        create(INVALID_ARGUMENT, first=first, count=count)
    create(SCENE, indices=bad_idx.handle)                                         # on any error nothing is allocated (live_resources, above)
    info = _lib.NormalsPlanInfo()
    refused(lib.urt_normals_plan_info(h, 0xdead, C.byref(info)), INVALID_HANDLE)
    refused(lib.urt_normals_plan_info(h, plan.handle, None), INVALID_ARGUMENT)
    refused(lib.urt_normals_plan_release(h, 0xdead), INVALID_HANDLE)
    refused(lib.urt_normals_plan_release(h, raw.V.handle), INVALID_HANDLE)
    # urt_compute_normals
    for p in (plan.handle, empty.handle):                                         # an empty plan is checked like any other
        refused(lib.urt_compute_normals(h, p, 0), INVALID_HANDLE, p)
        refused(lib.urt_compute_normals(h, p, 0xdead), INVALID_HANDLE, p)
        refused(lib.urt_compute_normals(h, p, other16.handle), INVALID_ARGUMENT, p)      # a stride that is not 12
        refused(lib.urt_compute_normals(h, p, other12.handle), INVALID_ARGUMENT, p)      # another count
        refused(lib.urt_compute_normals(h, p, raw.V.handle), INVALID_ARGUMENT, p)        # the vertices buffer itself
    refused(lib.urt_compute_normals(h, 0xdead, raw.D.handle), INVALID_HANDLE)
    refused(lib.urt_compute_normals(h, raw.D.handle, raw.D.handle), INVALID_HANDLE)      # a buffer is not a plan
    refused(lib.urt_compute_normals(h, empty.handle, raw.D.handle), 0)            # an empty plan: OK after the checks, nothing marked
    got = f32(raw.D)
    assert same(got[2:12], host_scene.compute_normals(v, t)[2:12]) and (got[:2] == SENTINEL).all() and (got[12:] == SENTINEL).all()
    # a plan whose vertices buffer was released
    state_d = gpu_ctx.buffer_state(raw.D)
    raw.V.Release()
    assert lib.urt_compute_normals(h, plan.handle, raw.D.handle) == INVALID_HANDLE and gpu_ctx.buffer_state(raw.D) == state_d
    assert plan.info["count"] == 10
    plan.Release(); empty.Release()
    assert plan.handle == 0
    for b in (raw.I, raw.D, other12, other16, bad_idx, odd_idx):
        b.Release()


def test_errors_leave_the_frame_untouched(gpu_ctx):
    sc = mixed(SMALL)
    try:
        m, _ = start(gpu_ctx, copy.copy(sc), 0, 2)
        want = frame(m)
        lib, h = gpu_ctx.lib, gpu_ctx._h
        plan = gpu_ctx.normals_plan(m._vertexBuffer, m._indexBuffer, 0, 98)
        out = C.c_uint64()
        p0 = gpu_ctx.refit_stats()[1]
        V, I, NB = m._vertexBuffer.handle, m._indexBuffer.handle, m._normalBuffer.handle
        for call, code in ((lambda: lib.urt_normals_plan_create(h, V, I, 140, 9, C.byref(out)), INVALID_ARGUMENT),
                           (lambda: lib.urt_normals_plan_create(h, V, NB, 0, 98, C.byref(out)), INVALID_ARGUMENT),
                           (lambda: lib.urt_normals_plan_create(h, 0, I, 0, 98, C.byref(out)), INVALID_HANDLE),
                           (lambda: lib.urt_compute_normals(h, plan.handle, V), INVALID_ARGUMENT),
                           (lambda: lib.urt_compute_normals(h, plan.handle, I), INVALID_ARGUMENT),
                           (lambda: lib.urt_compute_normals(h, plan.handle, 0), INVALID_HANDLE),
                           (lambda: lib.urt_compute_normals(h, 0xdead, NB), INVALID_HANDLE)):
            assert call() == code
            assert bits_equal(frame(m), want) and gpu_ctx.refit_stats()[1] == p0  # after each: nothing was dirtied, no preparation
        plan.Release()
        m.OnDisable()
    finally:
        restore(gpu_ctx)


# ---- 6. a stale plan is safe ------------------------------------------------------------------------------------------------------------
def test_a_plan_keeps_its_own_triangles(gpu_ctx):
    v, t = scenes.uv_blob(12, 9)
    t = t.reshape(-1).astype(np.int32)
    raw = Raw(gpu_ctx, v, t)
    old = N.plan(v, t, 3, 80)
    plan = gpu_ctx.normals_plan(raw.V, raw.I, 3, 80)
    other = t.reshape(-1, 3)[::-1][:, [1, 2, 0]].reshape(-1).copy()               # other, valid indices: another slot order, other faces first
    other[:30] = 0
    assert not np.array_equal(N.plan(v, other, 3, 80)["entries"], old["entries"])
    raw.I.SetData(other)
    w = N.wobble(v, 0.9)
    raw.V.SetData(w)
    plan.compute(raw.D)
    assert same(f32(raw.D)[3:83], N.apply(old, w))                                # the OLD plan, on the current positions
    assert plan.info["n_triangles"] == len(old["tris"])
    plan.Release(); raw.release()


# ---- 7. resources -----------------------------------------------------------------------------------------------------------------------
def test_resources_return_to_the_baseline(gpu_ctx):
    gpu_ctx.synchronize()
    outer = live_resources()
    v, t = N.seam_sphere()
    with Context(gpu_ctx.device) as ctx:
        raw = Raw(ctx, v, t)
        warm = ctx.normals_plan(raw.V, raw.I)                                     # the mirrors and the face scratch are made once
        warm.compute(raw.D)
        warm.Release()
        base = live_resources()
        plan = ctx.normals_plan(raw.V, raw.I, 1, 20)
        assert live_resources()["device_bytes"] == base["device_bytes"] + plan.info["device_bytes"] and plan.info["device_bytes"] > 0
        plan.compute(raw.D)
        plan.Release()
        assert live_resources() == base
        kept = ctx.normals_plan(raw.V, raw.I)                                     # alive when its buffers and then the context go
        kept.compute(raw.D)
        raw.release()
        assert kept.info["count"] == len(v)
    assert live_resources() == outer
