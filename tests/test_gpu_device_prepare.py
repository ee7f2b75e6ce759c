"""GPU: full preparations fed from device memory (include/urt.h option "prepare_device"; csrc/scene_prep.cpp prepare_scene,
csrc/index_span.hip).  With the option on, a preparation from scratch — new topology, buffers of another count, a forced rebuild, the
in-place update switched off — takes _Vertices / _Indices / _Normals from the buffers' device mirrors: none of them is downloaded, the
triangle BVHs are built on the GPU and the MeshObjects' vertex spans are found there.  Pixels do not depend on the tree, so every frame
is checked bit for bit against a from-scratch preparation on a second context and against the oracle's literal walk; the spans against
the restatement of tests/deform_ref.py.  With the option off nothing has moved: the same scenario downloads each buffer once."""
import contextlib
import copy

import numpy as np
import pytest

import deform_ref as D
import skin_ref as S
from oracle import pyoracle
from test_gpu_buffer_device import dev, downloads
from test_gpu_deform import N_BLOB, SMALL, frame, mixed, other_ctx, restore, start, stats  # noqa: F401  (other_ctx: a fixture)
from test_gpu_refit import bits_equal, fresh_frame
from test_gpu_skin import RawSkin, bend, f32, posed, same
from unityraytracer_amd import ComputeBuffer, RayTraceMaster, scenes

pytestmark = pytest.mark.gpu

F = np.float32
NB = N_BLOB[(12, 9)]
OTHER_BLOB = (10, 7)                                       # another tessellation: vertex, normal and index counts all differ from mixed()'s
INT32_MAX = 2 ** 31 - 1
_REFERENCE = {}


def reference(key, ctx, sc):
    """(the frame of a from-scratch preparation on the second context, the oracle's) — rendered once per scene and shared."""
    if key not in _REFERENCE:
        _REFERENCE[key] = (fresh_frame(ctx, sc, 3), pyoracle.Oracle(sc).render(mode=0, threads=8))
    return _REFERENCE[key]


def other_tessellation():
    nxt = scenes.mixed_test_scene(96, 64, blob=OTHER_BLOB)
    sc = mixed()
    assert len(nxt.mesh_objects) == len(sc.mesh_objects) and len(nxt.mesh_bvh) == len(sc.mesh_bvh)
    assert len(nxt.vertices) != len(sc.vertices) and len(nxt.indices) != len(sc.indices) and len(nxt.normals) != len(sc.normals)
    return nxt


def geometry(m):
    return (m._vertexBuffer, m._indexBuffer, m._normalBuffer)


def prepared(ctx):
    """(full preparations, those fed from device memory, preparations in place, MeshObjects refitted) so far."""
    p = ctx.prepare_stats()
    refitted, in_place = ctx.refit_stats()
    return np.array([p["full"], p["device"], in_place, refitted])


def rebind(ctx, m, nxt, on_device=(True, True, True)):
    """The geometry of `nxt` in FRESH ComputeBuffers — on_device: SetDataDevice is their first and only write; else a host SetData —
    bound in place of the master's; the small tables through SetData."""
    olds = geometry(m)
    news = []
    for data, stride, device in zip((nxt.vertices, nxt.indices, nxt.normals), (12, 4, 12), on_device):
        data = np.ascontiguousarray(data)
        buf = ComputeBuffer(ctx, len(data), stride)
        if device:
            buf.SetDataDevice(dev(data))
        else:
            buf.SetData(data)
        news.append(buf)
    ctx.synchronize()                                        # (the source tensors are dropped: the copies have read them)
    m._vertexBuffer, m._indexBuffer, m._normalBuffer = news
    m._meshObjectBuffer.SetData(nxt.mesh_objects)
    m._meshObjectBVHBuffer.SetData(nxt.mesh_bvh)
    for b in olds:
        b.Release()


@contextlib.contextmanager
def new_topology(ctx, other, builder, option):
    sc, nxt = mixed(), other_tessellation()
    try:
        ctx.set_option("prepare_device", option)
        m, _ = start(ctx, copy.copy(sc), builder)
        before = prepared(ctx)
        rebind(ctx, m, nxt)
        got = frame(m)
        fresh, oracle = reference("other", other, nxt)
        print("downloads", [ctx.buffer_state(b)["downloads"] for b in geometry(m)], "prepared", prepared(ctx) - before,
              "builder", ctx.launch_info()["blas_builder"])
        assert bits_equal(got, fresh) and bits_equal(got, oracle)
        assert (prepared(ctx) - before).tolist() == [1, option, 0, 0]           # one preparation from scratch, nothing in place, nothing refitted
        yield m, nxt
        m.OnDisable()
        ctx.synchronize()
    finally:
        ctx.set_option("prepare_device", 0)
        restore(ctx)


# ---- 1. new topology from device memory ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [-1, 0, 1, 3])
def test_new_topology_from_device_memory(gpu_ctx, other_ctx, builder):
    with new_topology(gpu_ctx, other_ctx, builder, 1) as (m, nxt):
        assert downloads(gpu_ctx, *geometry(m)) == 0
        assert gpu_ctx.launch_info()["blas_builder"] == (builder if builder >= 1 else 3)      # always a GPU builder: the one asked for, else 3
        assert gpu_ctx.scene_info()["n_tris"] == len(nxt.indices) // 3
        for b in geometry(m):                                                     # the host copies were never read: still stale as a whole
            st = gpu_ctx.buffer_state(b)
            assert (st["stale_first"], st["stale_last"]) == (0, b.count - 1)
        assert same(f32(m._vertexBuffer), nxt.vertices) and downloads(gpu_ctx, m._vertexBuffer) == 1      # GetData is the first download
        assert downloads(gpu_ctx, m._indexBuffer, m._normalBuffer) == 0


# ---- 7. the option off: the default has not moved ---------------------------------------------------------------------------------------
def test_option_off_downloads_each_buffer_once(gpu_ctx, other_ctx):
    with new_topology(gpu_ctx, other_ctx, 3, 0) as (m, nxt):
        assert [gpu_ctx.buffer_state(b)["downloads"] for b in geometry(m)] == [1, 1, 1]
        assert gpu_ctx.launch_info()["blas_builder"] == 3
        assert same(f32(m._vertexBuffer), nxt.vertices) and downloads(gpu_ctx, m._vertexBuffer) == 1      # the host copy is current


# ---- 2. same counts, _Indices rewritten on the device -----------------------------------------------------------------------------------
def test_indices_rewritten_on_the_device(gpu_ctx, other_ctx):
    sc = mixed()
    try:
        gpu_ctx.set_option("prepare_device", 1)
        m, _ = start(gpu_ctx, copy.copy(sc), 3)
        first = frame(m)
        n0 = int(sc.mesh_objects[0]["indices_count"])
        assert int(sc.mesh_objects[0]["indices_offset"]) == 0 and n0 % 3 == 0
        # the triangles of the blob in another order: the same surface
        rolled = sc.indices.copy()
        rolled[:n0] = np.roll(sc.indices[:n0].reshape(-1, 3), 7, axis=0).reshape(-1)
        before = prepared(gpu_ctx)
        t = dev(rolled)                                      # (kept until the frame has been read back: the copy is enqueued, not waited for)
        m._indexBuffer.SetDataDevice(t)
        got = frame(m)
        print("rolled: prepared", prepared(gpu_ctx) - before, "downloads", downloads(gpu_ctx, *geometry(m)))
        assert (prepared(gpu_ctx) - before).tolist() == [1, 1, 0, 0] and downloads(gpu_ctx, *geometry(m)) == 0
        assert bits_equal(got, first)
        # a handful of its triangles wound the other way: another surface, the oracle's
        turned = rolled.copy()
        tri = turned[:n0].reshape(-1, 3)
        tri[::8] = tri[::8][:, [0, 2, 1]]
        nxt = copy.copy(sc)
        nxt.indices = turned
        before = prepared(gpu_ctx)
        t = dev(turned)
        m._indexBuffer.SetDataDevice(t)
        got = frame(m)
        assert (prepared(gpu_ctx) - before).tolist() == [1, 1, 0, 0] and downloads(gpu_ctx, *geometry(m)) == 0
        assert not bits_equal(got, first)
        assert bits_equal(got, pyoracle.Oracle(nxt).render(mode=0, threads=8))
        assert bits_equal(got, fresh_frame(other_ctx, nxt, 3))
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        gpu_ctx.set_option("prepare_device", 0)
        restore(gpu_ctx)


# ---- 3. the fallbacks of tests/test_gpu_buffer_device.py, with the option on ----------------------------------------------------------
@pytest.mark.parametrize("case", ["refit_vertices0", "refit0", "rebuild_pct", "bound_afterwards", "another_count"])
def test_fallbacks_read_the_device_written_data_in_place(gpu_ctx, other_ctx, case):
    sc = mixed()
    raw = None
    try:
        gpu_ctx.set_option("prepare_device", 1)
        m, _ = start(gpu_ctx, copy.copy(sc), 0)
        idx, wgt, bones, _ = bend(sc, SMALL)
        if case == "rebuild_pct":                                                 # a violent pose: the refitted tree is abandoned
            gpu_ctx.set_option("refit_rebuild_pct", 101)
            bones = S.two_bone_bend(sc.vertices[:NB], 175.0)[2]
            bones[1, :9] *= np.array([6, 6, 6, 0.2, 0.2, 0.2, 5, 5, 5], F)
        if case == "refit0":
            gpu_ctx.set_option("refit", 0)
            m.OnRenderImage()
        if case == "refit_vertices0":
            gpu_ctx.set_option("refit_vertices", 0)
        d0, (r0, p0), _ = stats(gpu_ctx)
        before = prepared(gpu_ctx)
        if case in ("bound_afterwards", "another_count"):
            extra = 3 if case == "another_count" else 0
            rest_v = np.concatenate([sc.vertices, np.zeros((extra, 3), F)])
            rest_n = np.concatenate([sc.normals, np.zeros((extra, 3), F)])
            j4, w4 = np.zeros((len(rest_v), 4), np.int32), np.zeros((len(rest_v), 4), F)
            j4[:NB], w4[:NB] = idx, wgt
            raw = RawSkin(gpu_ctx, rest_v, rest_n, j4, w4, bones)
            raw.dst_v.SetData(rest_v); raw.dst_n.SetData(rest_n)
            raw.skin(0, NB)
            nxt = posed(sc, NB, idx, wgt, bones)
            nxt.vertices = np.concatenate([nxt.vertices, np.zeros((extra, 3), F)])
            nxt.normals = np.concatenate([nxt.normals, np.zeros((extra, 3), F)])
            olds = (m._vertexBuffer, m._normalBuffer)
            m._vertexBuffer, m._normalBuffer = raw.dst_v, raw.dst_n              # the next frame binds them: a full preparation
            m._meshObjectBVHBuffer.SetData(nxt.mesh_bvh)
            for b in olds:
                b.Release()
        else:
            m.AttachSkin(0, idx, wgt)
            m.SkinMeshes({0: bones})
            nxt = posed(sc, NB, idx, wgt, bones, heap=m.scene.mesh_bvh)
        got = frame(m)
        d1, (r1, p1), _ = stats(gpu_ctx)
        print(case, "downloads", downloads(gpu_ctx, *geometry(m)), "prepared", prepared(gpu_ctx) - before)
        assert downloads(gpu_ctx, *geometry(m)) == 0, case                        # nothing came down for the full preparation
        assert (d1["deformed"], r1, p1) == (d0["deformed"], r0, p0), case         # nothing in place
        assert (prepared(gpu_ctx) - before)[:2].tolist() == [1, 1], case
        assert d1["forced_rebuilds"] - d0["forced_rebuilds"] == (1 if case == "rebuild_pct" else 0)
        assert bits_equal(got, fresh_frame(other_ctx, nxt, 0)), case
        st = gpu_ctx.buffer_state(m._vertexBuffer)
        assert (st["stale_first"], st["stale_last"]) == (0, NB - 1), case         # the host copy is still behind where the skin wrote
        assert same(f32(m._vertexBuffer), nxt.vertices) and downloads(gpu_ctx, m._vertexBuffer) == 1      # and GetData downloads as it always did
        m.OnDisable()
        if raw is not None:
            for b in (raw.rest_v, raw.rest_n, raw.idx, raw.wgt, raw.bones):
                b.Release()
        gpu_ctx.synchronize()
    finally:
        gpu_ctx.set_option("prepare_device", 0)
        restore(gpu_ctx)


# ---- 4. the spans ---------------------------------------------------------------------------------------------------------------------------
def fan_scene(chunk):
    """Small fans over a pool of random points whose MeshObjects exercise the edges of csrc/index_span.hip: see the table below.
    -> (scene, the names of the MeshObjects)."""
    rng = np.random.default_rng(31)
    nv = 300
    vertices = (rng.uniform(-1.0, 1.0, (nv, 3)) * np.array([1.5, 1.0, 1.5]) + np.array([0.0, 1.3, 0.0])).astype(F)

    def fan(n_indices, first=None, last=None):
        """n_indices index slots of triangles with three distinct vertices from the pool's interior; `first` / `last` replace the first /
        the last slot of the whole triangles."""
        tris = np.array([rng.choice(np.arange(5, nv - 5), 3, replace=False) for _ in range((n_indices + 2) // 3)], np.int32).reshape(-1)[:n_indices]
        whole = n_indices // 3 * 3
        if first is not None:
            tris[0] = first
        if last is not None:
            tris[whole - 1] = last
        return tris

    long = 3 * chunk + 6                                     # its pieces end at chunk, 2 chunk and 3 chunk: every residue mod 3 a piece boundary can have
    ranges = [                                               # name, index slots, the MeshObjects that share the range
        ("long", fan(long, first=0, last=nv - 1), 1),        # index 0 at the first and n_vertices - 1 at the last scanned slot
        ("pad1", fan(1), 0),                                 # (a slot no MeshObject names: the ranges behind it start at another alignment)
        ("chunk+1tri", fan(chunk + 3), 1),                   # one triangle longer than a chunk
        ("shared", fan(36), 2),                              # two MeshObjects, one range
        ("five", np.concatenate([fan(3), [0, nv - 1]]).astype(np.int32), 1),      # the remainder is not scanned: it would widen the span
        ("pad2", fan(2), 0),
        ("four", np.concatenate([fan(3), [nv - 1]]).astype(np.int32), 1),
        ("two", np.array([0, nv - 1], np.int32), 1),         # fewer than three indices: no span
        ("one", fan(3), 1),                                  # one triangle
        ("zero", np.zeros(0, np.int32), 1),
    ]
    indices = np.concatenate([r[1] for r in ranges]).astype(np.int32)
    offsets = np.cumsum([0] + [len(r[1]) for r in ranges])
    names, records = [], []
    for k in reversed(range(len(ranges))):                   # descending offsets
        for _ in range(ranges[k][2]):
            mo = np.zeros((), scenes.MESHOBJECT_DT)
            mo["localToWorldMatrix"], mo["indices_offset"], mo["indices_count"] = scenes.trs(), offsets[k], len(ranges[k][1])
            mo["lighting"] = scenes._params((0.6, 0.5, 0.4), (0.1, 0.1, 0.1), (0, 0, 0), 0.3)
            records.append(mo); names.append(ranges[k][0])
    mesh_objects = np.array(records, scenes.MESHOBJECT_DT)
    lo, hi = np.zeros((len(mesh_objects), 3), F), np.zeros((len(mesh_objects), 3), F)      # (an empty box for a MeshObject without a triangle)
    for m, mo in enumerate(mesh_objects):
        if mo["indices_count"] >= 3:
            whole = copy.copy(mo); whole["indices_count"] = mo["indices_count"] // 3 * 3
            l1, h1 = scenes.mesh_bounds(np.array([whole], scenes.MESHOBJECT_DT), vertices, indices)
            lo[m], hi[m] = l1[0], h1[0]
    sc = scenes.Scene("fans", 96, 64, 2, 1, mesh_objects=mesh_objects, vertices=vertices, indices=indices,
                      normals=scenes.compute_normals(vertices, indices), mesh_bvh=scenes.build_object_bvh(lo, hi), sky=scenes.make_sky(64, 32))
    return sc, names


def test_vertex_spans_from_the_device(gpu_ctx):
    chunk = gpu_ctx.prepare_stats()["span_chunk"]            # the kernel's constant, from the library
    assert 3 <= chunk <= 1 << 16
    sc, names = fan_scene(chunk)
    n = len(sc.mesh_objects)
    assert sorted(set(names)) == sorted({"long", "chunk+1tri", "shared", "five", "four", "two", "one", "zero"}) and names.count("shared") == 2
    assert (np.diff(sc.mesh_objects["indices_offset"]) <= 0).all() and len({int(o) % 4 for o in sc.mesh_objects["indices_offset"]}) == 4
    want_lo, want_hi = D.vertex_spans(sc.mesh_objects, sc.indices)
    none = want_lo > want_hi
    want_lo = np.where(none, INT32_MAX, want_lo)             # the library's "no span" (include/urt.h urt_debug_scene_vertex_spans)
    assert [names[m] for m in np.nonzero(none)[0]] == ["zero", "two"]
    k = names.index("long")
    assert (want_lo[k], want_hi[k]) == (0, len(sc.vertices) - 1)
    for name in ("five", "four"):
        assert 0 < want_lo[names.index(name)] and want_hi[names.index(name)] < len(sc.vertices) - 1
    try:
        gpu_ctx.set_option("kernel_mode", 3); gpu_ctx.set_option("blas_leaf_max", 2); gpu_ctx.set_option("blas_builder", 3)
        gpu_ctx.set_option("prepare_device", 1)
        m = RayTraceMaster(gpu_ctx, sc)
        m._scene_ready()
        t = dev(sc.indices)
        m._indexBuffer.SetDataDevice(t)                      # read from the mirror
        before = prepared(gpu_ctx)
        m.OnRenderImage()
        lo, hi = gpu_ctx.scene_vertex_spans(n)
        print("device", list(zip(names, lo.tolist(), hi.tolist())))
        assert (prepared(gpu_ctx) - before).tolist() == [1, 1, 0, 0] and downloads(gpu_ctx, *geometry(m)) == 0
        assert lo.dtype == np.int32 and np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)
        with pytest.raises(Exception):
            gpu_ctx.scene_vertex_spans(n + 1)
        gpu_ctx.set_option("prepare_device", 0)              # stale: the host loop over the downloaded _Indices
        lo, hi = gpu_ctx.scene_vertex_spans(n)
        print("host", list(zip(names, lo.tolist(), hi.tolist())))
        assert (prepared(gpu_ctx) - before).tolist() == [2, 1, 0, 0] and downloads(gpu_ctx, m._indexBuffer) == 1
        assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)
        gpu_ctx.set_option("refit", 0)                       # nothing is kept
        lo, hi = gpu_ctx.scene_vertex_spans(n)
        assert (lo == INT32_MAX).all() and (hi == -1).all()
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        gpu_ctx.set_option("prepare_device", 0)
        restore(gpu_ctx)


# ---- 5. in place afterwards ---------------------------------------------------------------------------------------------------------------
def test_in_place_after_a_device_preparation(gpu_ctx, other_ctx):
    sc = mixed()
    try:
        gpu_ctx.set_option("prepare_device", 1)
        m, _ = start(gpu_ctx, copy.copy(sc), 3)
        lo, hi = gpu_ctx.scene_vertex_spans(3)
        assert (lo[0], hi[0]) == (0, NB - 1) and lo[1] == NB
        nxt = bend(sc, SMALL)[3]
        before = prepared(gpu_ctx)
        d0 = gpu_ctx.deform_stats()
        tv, tn = dev(nxt.vertices[:NB]), dev(nxt.normals[:NB])
        m._vertexBuffer.SetDataDevice(tv, 0, NB)                                  # meets the blob's span only
        m._normalBuffer.SetDataDevice(tn, 0)
        m._meshObjectBVHBuffer.SetData(nxt.mesh_bvh)
        got = frame(m)
        d1 = gpu_ctx.deform_stats()
        print("prepared", prepared(gpu_ctx) - before, "deformed", d1["deformed"] - d0["deformed"])
        assert (d1["deformed"] - d0["deformed"], d1["renormed"] - d0["renormed"]) == (1, 1)
        assert (prepared(gpu_ctx) - before).tolist() == [0, 0, 1, 1]             # no preparation from scratch: one in place, one MeshObject refitted
        assert downloads(gpu_ctx, *geometry(m)) == 0
        assert bits_equal(got, fresh_frame(other_ctx, nxt, 3))
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        gpu_ctx.set_option("prepare_device", 0)
        restore(gpu_ctx)


# ---- 6. mixed sources ---------------------------------------------------------------------------------------------------------------------
def test_mixed_sources(gpu_ctx, other_ctx):
    sc, nxt = mixed(), other_tessellation()
    try:
        gpu_ctx.set_option("prepare_device", 1)
        m, _ = start(gpu_ctx, copy.copy(sc), 3)
        before = prepared(gpu_ctx)
        rebind(gpu_ctx, m, nxt, on_device=(True, False, False))                   # _Vertices has a mirror; _Indices / _Normals are host-set and have none
        got = frame(m)
        fresh, oracle = reference("other", other_ctx, nxt)
        assert [gpu_ctx.buffer_state(b)["mirror_bytes"] for b in geometry(m)] == [len(nxt.vertices) * 12, 0, 0]
        assert (prepared(gpu_ctx) - before).tolist() == [1, 1, 0, 0] and downloads(gpu_ctx, *geometry(m)) == 0
        assert bits_equal(got, fresh) and bits_equal(got, oracle)
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        gpu_ctx.set_option("prepare_device", 0)
        restore(gpu_ctx)


# ---- 8. RayTraceMaster.ReplaceGeometryDevice -------------------------------------------------------------------------------------------
def test_replace_geometry_device(gpu_ctx, other_ctx):
    sc, nxt = mixed(), other_tessellation()
    try:
        gpu_ctx.set_option("kernel_mode", 3); gpu_ctx.set_option("blas_leaf_max", 2); gpu_ctx.set_option("blas_builder", -1)
        m = RayTraceMaster(gpu_ctx, copy.copy(sc))
        m.device_object_heaps = True
        m.device_prepare = True
        m.EnableTemporalAccumulation()
        for _ in range(3):
            m.OnRenderImage()
        assert (m._tcount.GetPixels()[..., 0] == 3).all()
        before = prepared(gpu_ctx)
        tv, ti, tn = dev(nxt.vertices), dev(nxt.indices), dev(nxt.normals)
        m.ReplaceGeometryDevice(tv, (ti.data_ptr(), len(nxt.indices)), tn, nxt.mesh_objects)      # a tensor, a raw address with its count
        gpu_ctx.synchronize()
        assert m._currentSample == 0 and [b.count for b in geometry(m)] == [len(nxt.vertices), len(nxt.indices), len(nxt.normals)]
        m.OnRenderImage()
        got = m._target.GetPixels()
        assert (m._tcount.GetPixels()[..., 0] == 1).all()                         # the count texture restarted
        assert bits_equal(m._converged.GetPixels()[..., :3], got[..., :3])       # ... and the mean with it
        assert (prepared(gpu_ctx) - before).tolist() == [1, 1, 0, 0] and downloads(gpu_ctx, *geometry(m)) == 0
        other_ctx.set_option("kernel_mode", 3); other_ctx.set_option("blas_builder", 3)
        m2 = RayTraceMaster(other_ctx, copy.copy(nxt))                            # a master made from the new scene, at the same frame
        m2._frame = m._frame - 1
        m2.OnRenderImage()
        assert bits_equal(got, m2._target.GetPixels())
        m2.OnDisable()
        # the same buffers again (their counts fit: reused), with the heap given
        olds = geometry(m)
        m.ReplaceGeometryDevice(tv, ti, tn, nxt.mesh_objects, nxt.mesh_bvh)
        gpu_ctx.synchronize()
        assert geometry(m) == olds
        m.SyncGeometry()
        assert same(m.scene.vertices, nxt.vertices) and np.array_equal(m.scene.indices, nxt.indices) and same(m.scene.normals, nxt.normals)
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        gpu_ctx.set_option("prepare_device", 0)
        restore(gpu_ctx)
