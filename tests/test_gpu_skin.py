"""GPU: skinning on the device (include/urt.h urt_skin_vertices, urt_buffer_bounds; csrc/skin.hip) and RayTraceMaster.AttachSkin /
SkinMeshes on top of it.  The kernel is held to the numpy restatement of tests/skin_ref.py bit for bit (a NaN equals a NaN: its sign and
payload are not arithmetic, and the host's and the device's default NaN differ); frames after a skinned update are held, bit for bit, to
a from-scratch preparation of the restatement's vertices and normals on a second context and to the oracle's literal walk, and the
counters show that the positions never touched the host."""
import copy
import ctypes as C

import numpy as np
import pytest

import deform_ref as D
import refit_ref as R
import skin_ref as S
from oracle import pyoracle
from test_gpu_deform import DEEP, N_BLOB, SMALL, frame, mixed, other_ctx, restore, start, stats, with_vertices  # noqa: F401  (other_ctx: a fixture)
from test_gpu_refit import bits_equal, fresh_frame
from unityraytracer_amd import ComputeBuffer, Context, RayTraceMaster, _lib, live_resources, scenes

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = F(7.5)
INVALID_ARGUMENT, INVALID_HANDLE = 1, 2


def same(a, b):
    """Bit for bit, a NaN equal to a NaN."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def f32(buf, first=0, count=None):
    return buf.GetData(first, count).view(F).reshape(-1, buf.stride // 4)


class RawSkin:
    """The five input buffers of urt_skin_vertices and two destinations filled with a sentinel, all of `n` elements."""

    def __init__(self, ctx, rest_v, rest_n, idx, wgt, bones):
        n = len(rest_v)
        self.ctx, self.n = ctx, n
        self.rest_v, self.rest_n = ComputeBuffer(ctx, n, 12), ComputeBuffer(ctx, n, 12)
        self.idx, self.wgt = ComputeBuffer(ctx, n, 16), ComputeBuffer(ctx, n, 16)
        self.bones = ComputeBuffer(ctx, len(bones), 48)
        self.dst_v, self.dst_n = ComputeBuffer(ctx, n, 12), ComputeBuffer(ctx, n, 12)
        for b, a in ((self.rest_v, rest_v), (self.rest_n, rest_n), (self.idx, idx), (self.wgt, wgt), (self.bones, bones)):
            b.SetData(np.ascontiguousarray(a))
        self.reset()

    def reset(self):
        for b in (self.dst_v, self.dst_n):
            b.SetData(np.full((self.n, 3), SENTINEL, F))

    def skin(self, first, count, normals=True):
        self.ctx.skin_vertices(self.rest_v, self.rest_n if normals else None, self.idx, self.wgt, self.bones, first, count, self.dst_v,
                               self.dst_n if normals else None)

    def all(self):
        return (self.rest_v, self.rest_n, self.idx, self.wgt, self.bones, self.dst_v, self.dst_n)

    def release(self):
        for b in self.all():
            b.Release()


def variant_case(variant, n, n_bones, seed):
    rng = np.random.default_rng(seed)
    P = rng.uniform(-3, 3, (n, 3)).astype(F)
    N = rng.normal(size=(n, 3)).astype(F)
    j = rng.integers(0, n_bones, (n, 4)).astype(np.int32)
    w = rng.uniform(0, 1, (n, 4)).astype(F)
    w = (w / w.sum(axis=1, keepdims=True)).astype(F)
    A = rng.uniform(-1.5, 1.5, (n_bones, 12)).astype(F)
    if variant == "zero_wild":                               # zero weights with wild indices
        dead = rng.random((n, 4)) < 0.4
        w[dead] = 0
        j[dead] = rng.choice(np.array([10 ** 9, -10 ** 9, 2 ** 31 - 1, -2 ** 31, n_bones], np.int64), int(dead.sum())).astype(np.int32)
        w[0] = 0                                             # (all four dead: +0 and a zero normal)
    elif variant == "negative":                              # negative and too-large indices under weights that are not zero
        bad = rng.random((n, 4)) < 0.3
        j[bad] = rng.choice(np.array([-1, -7, n_bones, n_bones + 1, 10 ** 9], np.int64), int(bad.sum())).astype(np.int32)
    elif variant == "unnormalised":
        w = rng.uniform(-2, 3, (n, 4)).astype(F)
    elif variant == "nan_weight":
        w[rng.random((n, 4)) < 0.1] = np.nan
        w[n // 2, 1] = np.nan
    elif variant == "inf_bone":
        A[0, 4] = np.inf
        A[n_bones - 1, 10] = -np.inf
    else:
        assert variant == "plain"
    return P, N, j, w, A


VARIANTS = ("plain", "zero_wild", "negative", "unnormalised", "nan_weight", "inf_bone")


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bones", [1, 3, 300])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, 1202])
def test_skin_vertices_equals_the_restatement(gpu_ctx, count, n_bones):
    assert 3 <= S.LDS_BONES < 300                            # 1 and 3 bones are staged in LDS, 300 are gathered from global memory
    for vi, variant in enumerate(VARIANTS):
        for first in (0, 5):
            n = first + count + 3
            P, N, j, w, A = variant_case(variant, n, n_bones, seed=1000 * vi + count + first)
            want_v, want_n = S.skin(P, N, j, w, A)
            raw = RawSkin(gpu_ctx, P, N, j, w, A)
            for normals in (True, False):
                raw.reset()
                raw.skin(first, count, normals)
                state = gpu_ctx.buffer_state(raw.dst_v)
                assert (state["stale_first"], state["stale_last"], state["mirror_bytes"]) == (first, first + count - 1, n * 12)
                got_v, got_n = f32(raw.dst_v), f32(raw.dst_n)
                what = (variant, first, count, n_bones, normals)
                inside = slice(first, first + count)
                assert same(got_v[inside], want_v[inside]), what
                assert same(got_n[inside], want_n[inside] if normals else np.full((count, 3), SENTINEL, F)), what
                outside = np.ones(n, bool); outside[inside] = False
                assert (got_v[outside] == SENTINEL).all() and (got_n[outside] == SENTINEL).all(), what
            raw.release()


# ---- 2. frames --------------------------------------------------------------------------------------------------------------------------
def bend(sc, size, angle=40.0):
    """A two-bone bend of the blob: (indices, weights, bones) and the scene the restatement makes of it (the heap is filled in later)."""
    nb = N_BLOB[size[1]]
    idx, wgt, bones = S.two_bone_bend(sc.vertices[:nb], angle)
    return idx, wgt, bones, posed(sc, nb, idx, wgt, bones)


def posed(sc, nb, idx, wgt, bones, heap=None):
    v, n = S.skin(sc.vertices[:nb], sc.normals[:nb], idx, wgt, bones)
    vertices, normals = sc.vertices.copy(), sc.normals.copy()
    vertices[:nb], normals[:nb] = v, n
    out = with_vertices(sc, vertices, normals=normals, heap=heap is None)
    if heap is not None:
        out.mesh_bvh = heap
    return out


def check_skinned_frame(ctx, other, m, builder, sc, nxt, nodes, tri, root, what, oracle=True):
    got = frame(m)
    new, tri2, root2, _ = ctx.read_scene_blas(len(sc.mesh_objects))
    assert np.array_equal(tri2, tri) and np.array_equal(root2, root), what
    want, _ = R.refit(nxt, nodes, tri, root, np.array([True, False, False]))
    assert bits_equal(new, want), f"{what}: refitted nodes differ from the restatement"
    assert bits_equal(got, fresh_frame(other, nxt, builder)), f"{what}: frame differs from a from-scratch preparation"
    if oracle:
        assert bits_equal(got, pyoracle.Oracle(nxt).render(mode=0, threads=8)), f"{what}: frame differs from the oracle's literal walk"
    return new


@pytest.mark.parametrize("size,builder,leaf", [(SMALL, b, l) for b in (0, 1, 3) for l in (1, 2, 8)] + [(DEEP, b, 2) for b in (0, 3)])
def test_skinned_frames(gpu_ctx, other_ctx, size, builder, leaf):
    sc = mixed(size)
    nb = N_BLOB[size[1]]
    try:
        m, (nodes, tri, root) = start(gpu_ctx, copy.copy(sc), builder, leaf)
        idx, wgt, bones, _ = bend(sc, size)
        m.AttachSkin(0, idx, wgt)
        spans = D.vertex_spans(sc.mesh_objects, sc.indices)
        deformed = D.meets(spans, (0, nb - 1))
        assert deformed.tolist() == [True, False, False]
        for step, angle in enumerate((40.0, -25.0, 70.0)):                        # three consecutive skinned frames
            bones = S.two_bone_bend(sc.vertices[:nb], angle)[2]
            d0, (r0, p0), built0 = stats(gpu_ctx)
            m.SkinMeshes({0: bones})
            assert m._currentSample == 0
            nxt = posed(sc, nb, idx, wgt, bones, heap=m.scene.mesh_bvh)
            nodes = check_skinned_frame(gpu_ctx, other_ctx, m, builder, sc, nxt, nodes, tri, root, f"{size} builder {builder} leaf {leaf} step {step}",
                                        oracle=step == 0)
            d1, (r1, p1), built1 = stats(gpu_ctx)
            assert (d1["deformed"] - d0["deformed"], d1["renormed"] - d0["renormed"], r1 - r0, p1 - p0) == (1, 1, 1, 1), (d0, d1)
            assert d1["bytes_copied"] - d0["bytes_copied"] == 2 * nb * 12 and d1["forced_rebuilds"] == d0["forced_rebuilds"]
            assert builder != 0 or built1 == built0                               # the host builder's cache built nothing
            for buf in (m._vertexBuffer, m._normalBuffer):                        # the positions never touched the host
                st = gpu_ctx.buffer_state(buf)
                assert st["downloads"] == 0 and (st["stale_first"], st["stale_last"]) == (0, nb - 1), st
        assert bits_equal(np.asarray(m.scene.vertices), sc.vertices)              # the scene's lists keep what they held
        # the world box SkinMeshes derived from the GPU's bounds contains the skinned mesh
        leaf_box = [nd for nd in m.scene.mesh_bvh if nd["index"] == 0][0]
        w = scenes.world_vertices(nxt.mesh_objects[0], nxt.vertices, nxt.indices)
        assert (w >= leaf_box["vmin"].astype(np.float64)).all() and (w <= leaf_box["vmax"].astype(np.float64)).all()
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        restore(gpu_ctx)


# ---- 6. bounds --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 64, 65, 1202])
def test_buffer_bounds_equal_numpy(gpu_ctx, count):
    rng = np.random.default_rng(count)
    first = 7
    v = rng.uniform(-50, 50, (first + count + 5, 3)).astype(F)
    v[:first] = 1e6; v[first + count:] = -1e6                                     # outside the range: would show
    bad = rng.random(len(v)) < 0.2
    v[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(bad.sum()))
    v[first, 0] = -0.0
    buf = ComputeBuffer(gpu_ctx, len(v), 12)
    buf.SetData(v)
    lo, hi, n = gpu_ctx.buffer_bounds(buf, first, count)
    wlo, whi, wn = S.bounds(v, first, count)
    assert n == wn and np.array_equal(lo, wlo) and np.array_equal(hi, whi), (count, n, wn, lo, wlo, hi, whi)      # as values
    assert gpu_ctx.buffer_bounds(buf, first, 0)[2] == 0
    # a range of only-NaN elements
    v[first: first + count] = np.nan
    buf.SetData(v)
    lo, hi, n = gpu_ctx.buffer_bounds(buf, first, count)
    assert n == 0 and np.isposinf(lo).all() and np.isneginf(hi).all()
    assert gpu_ctx.buffer_state(buf)["downloads"] == 0
    buf.Release()


def test_bounds_after_a_skin_without_a_download(gpu_ctx):
    P, N, j, w, A = variant_case("plain", 1202, 3, seed=5)
    raw = RawSkin(gpu_ctx, P, N, j, w, A)
    raw.skin(100, 1000)
    lo, hi, n = gpu_ctx.buffer_bounds(raw.dst_v, 100, 1000)
    want = S.skin(P, N, j, w, A)[0]
    wlo, whi, wn = S.bounds(want, 100, 1000)
    assert n == wn == 1000 and np.array_equal(lo, wlo) and np.array_equal(hi, whi)
    lo, hi, n = gpu_ctx.buffer_bounds(raw.dst_v)                                  # the sentinel outside the skinned range takes part
    assert n == 1202 and (hi == np.maximum(whi, SENTINEL)).all()
    st = gpu_ctx.buffer_state(raw.dst_v)
    assert st["downloads"] == 0 and (st["stale_first"], st["stale_last"]) == (100, 1099)
    assert same(f32(raw.dst_v)[100:1100], want[100:1100]) and gpu_ctx.buffer_state(raw.dst_v)["downloads"] == 1
    raw.release()


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_everything_untouched(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx._h
    P, N, j, w, A = variant_case("plain", 40, 3, seed=9)
    raw = RawSkin(gpu_ctx, P, N, j, w, A)
    raw.skin(2, 10)                                                               # (a stale range to keep)
    other12, other16 = ComputeBuffer(gpu_ctx, 41, 12), ComputeBuffer(gpu_ctx, 41, 16)
    before = [gpu_ctx.buffer_state(b) for b in raw.all()]
    d0 = gpu_ctx.deform_stats()
    H = {k: getattr(raw, k).handle for k in ("rest_v", "rest_n", "idx", "wgt", "bones", "dst_v", "dst_n")}

    def call(first=0, count=5, null_in=False, **over):
        a = dict(H, **over)
        sb = _lib.SkinBuffers(a["rest_v"], a["rest_n"], a["idx"], a["wgt"], a["bones"])
        return lib.urt_skin_vertices(h, None if null_in else C.byref(sb), first, count, a["dst_v"], a["dst_n"])

    assert call(null_in=True) == INVALID_ARGUMENT
    for first, count in ((-1, 1), (0, -1), (36, 5), (40, 1), (2 ** 31 - 1, 2)):
        assert call(first, count) == INVALID_ARGUMENT, (first, count)
    assert call(rest_v=other12.handle) == INVALID_ARGUMENT                        # counts that do not fit
    assert call(idx=other16.handle) == INVALID_ARGUMENT
    assert call(dst_n=other12.handle) == INVALID_ARGUMENT
    assert call(idx=H["rest_v"]) == INVALID_ARGUMENT                              # strides that do not fit
    assert call(bones=H["wgt"]) == INVALID_ARGUMENT
    assert call(dst_v=H["idx"]) == INVALID_ARGUMENT
    assert call(dst_v=H["rest_v"]) == INVALID_ARGUMENT                            # a destination equal to an input
    assert call(dst_n=H["rest_n"]) == INVALID_ARGUMENT
    assert call(dst_n=H["dst_v"]) == INVALID_ARGUMENT                             # ... or to the other destination
    assert call(rest_n=0) == INVALID_ARGUMENT                                     # dst_normals without rest_normals
    for key in ("rest_v", "idx", "wgt", "bones", "dst_v"):
        assert call(**{key: 0}) == INVALID_HANDLE and call(**{key: 0xdead}) == INVALID_HANDLE, key
    assert call(dst_n=0xdead) == INVALID_HANDLE and call(rest_n=0xdead) == INVALID_HANDLE
    assert call(count=0) == 0 and call(rest_n=0, dst_n=0, count=0) == 0           # count == 0: OK after the checks
    assert call(count=0, dst_v=H["rest_v"]) == INVALID_ARGUMENT
    # urt_buffer_bounds
    out6, n = (C.c_float * 6)(), C.c_int(77)
    for first, count in ((-1, 1), (0, -1), (36, 5), (2 ** 31 - 1, 2)):
        assert lib.urt_buffer_bounds(h, H["dst_v"], first, count, out6, C.byref(n)) == INVALID_ARGUMENT
    assert lib.urt_buffer_bounds(h, H["idx"], 0, 1, out6, C.byref(n)) == INVALID_ARGUMENT      # a stride other than 12
    assert lib.urt_buffer_bounds(h, H["dst_v"], 0, 1, None, C.byref(n)) == INVALID_ARGUMENT
    assert lib.urt_buffer_bounds(h, 0xdead, 0, 1, out6, C.byref(n)) == INVALID_HANDLE
    assert lib.urt_buffer_bounds(h, H["dst_v"], 2, 10, out6, None) == 0 and n.value == 77      # out_n may be NULL
    out4 = (C.c_uint64 * 4)()
    assert lib.urt_debug_buffer_state(h, 0xdead, out4) == INVALID_HANDLE and lib.urt_debug_buffer_state(h, H["dst_v"], None) == INVALID_ARGUMENT
    assert [gpu_ctx.buffer_state(b) for b in raw.all()] == before and gpu_ctx.deform_stats() == d0
    want = S.skin(P, N, j, w, A)[0]
    got = f32(raw.dst_v)
    assert same(got[2:12], want[2:12]) and (got[:2] == SENTINEL).all() and (got[12:] == SENTINEL).all()
    raw.release(); other12.Release(); other16.Release()


# ---- 8. resources -----------------------------------------------------------------------------------------------------------------------
def test_resources_return_to_the_baseline(gpu_ctx):
    gpu_ctx.synchronize()
    base = live_resources()
    sc = mixed()
    with Context(gpu_ctx.device) as ctx:
        m, _ = start(ctx, copy.copy(sc), 0)
        idx, wgt, bones, _ = bend(sc, SMALL)
        m.AttachSkin(0, idx, wgt)
        m.SkinMeshes({0: bones})
        frame(m)
        assert ctx.deform_stats()["deformed"] == 1 and ctx.buffer_state(m._vertexBuffer)["mirror_bytes"] == len(sc.vertices) * 12
        assert live_resources()["device_bytes"] > base["device_bytes"]
        released = ComputeBuffer(ctx, 64, 12)
        ctx.buffer_bounds(released)
        with_mirror = live_resources()["device_bytes"]
        released.Release()                                                        # a release gives the mirror back
        assert live_resources()["device_bytes"] == with_mirror - 64 * 12
        m.OnDisable()
    gpu_ctx.set_option("blas_leaf_max", 2)
    assert live_resources() == base


# ---- 9. the temporal protocol -----------------------------------------------------------------------------------------------------------
def test_skin_meshes_with_temporal_accumulation(gpu_ctx, other_ctx):
    sc = mixed()
    try:
        m = RayTraceMaster(gpu_ctx, copy.copy(sc))
        m.EnableTemporalAccumulation()
        for _ in range(6):
            m.OnRenderImage()
        idx, wgt, bones, _ = bend(sc, SMALL)
        m.AttachSkin(0, idx, wgt)
        d0 = gpu_ctx.deform_stats()["deformed"]
        m.SkinMeshes({0: bones})
        count = m._tcount.GetPixels()[..., 0]
        ids = m._taov[1][2].GetPixels()[..., 0].view(np.int32)                    # the new feature buffers: object id
        kind = m._taov[1][1].GetPixels()[..., 3]
        on_blob = (ids == 0) & (kind == 3.0)                                      # urt_RayHit kind 3: a triangle; object: its MeshObject
        assert gpu_ctx.deform_stats()["deformed"] == d0 + 1 and on_blob.any()
        assert (count[on_blob] == 0).all()
        assert (count[~on_blob] > 0).mean() >= 0.9
        n = m.ResampleDisocclusions()
        assert n >= int(on_blob.sum())
        assert (m._tcount.GetPixels()[..., 0][on_blob] > 0).all()
        assert gpu_ctx.buffer_state(m._vertexBuffer)["downloads"] == 0
        m.OnDisable()
    finally:
        restore(gpu_ctx)
