"""GPU: meshes that change SHAPE.  A SetData that changes elements of _Vertices / _Normals (same counts, _Indices untouched) is taken in
place (csrc/scene_prep.cpp prepare_incremental, option "refit_vertices"): only the dirty element range goes to the device, the MeshObjects
whose vertex span it meets are refitted (csrc/refit.hip, the kernels of a matrix move) or get their shading normals gathered again
(k_refit_norms), and the cost of a deformed MeshObject's tree is measured (k_tree_cost, option "refit_rebuild_pct").  Pixels depend on
the tree only through its being valid, so everything is checked bit for bit: against a from-scratch preparation on a second context,
against the oracle's literal walk, and the refitted nodes against the restatement of tests/refit_ref.py / tests/deform_ref.py."""
import copy
import ctypes as C

import numpy as np
import pytest

import cones_ref as K
import deform_ref as D
import refit_ref as R
from oracle import pyoracle
from test_blas import validate
from test_gpu_refit import bits_equal, fresh_frame, moved_scene
from unityraytracer_amd import ComputeBuffer, Context, RayTraceMaster, live_resources, scenes
from unityraytracer_amd._lib import UrtError

pytestmark = pytest.mark.gpu

F = np.float32
RESTORE = {"blas_builder": -1, "blas_leaf_max": 2, "qnodes": 0, "blas_cones": -1, "kernel_mode": 3, "refit": 1, "refit_vertices": 1,
           "refit_rebuild_pct": 0, "frames_per_launch": 0}
N_BLOB = {(12, 9): 12 * 8 + 2, (40, 31): 40 * 30 + 2}
SMALL, DEEP = ((96, 64), (12, 9)), ((160, 104), (40, 31))


def restore(ctx):
    for k, v in RESTORE.items():
        ctx.set_option(k, v)


@pytest.fixture(scope="module")
def other_ctx():
    """A second context: from-scratch preparations (refit = 0) that leave the bindings of the context under test alone."""
    ctx = Context(0)
    ctx.set_option("refit", 0)
    yield ctx
    ctx.close()


def mixed(size=SMALL):
    (w, h), blob = size
    return scenes.mixed_test_scene(w, h, blob=blob)


def with_vertices(sc, vertices, normals=None, recompute=True, heap=True):
    """The scene with other vertex positions: normals recomputed (or given, or kept), the object-level heap rebuilt from the new bounds
    (heap=False, for positions that are not finite: it keeps the boxes it had — any heap will do, both sides render with the same)."""
    out = copy.copy(sc)
    out.vertices = np.ascontiguousarray(vertices, F)
    if normals is not None:
        out.normals = np.ascontiguousarray(normals, F)
    elif recompute:
        with np.errstate(all="ignore"):
            out.normals = scenes.compute_normals(out.vertices, sc.indices)
    if heap:
        out.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(sc.mesh_objects, out.vertices, sc.indices))
    return out


def blob_phase(sc, size, phase, bumps=0.12):
    v, t = scenes.uv_blob(*size[1], bumps=bumps, phase=phase)
    assert np.array_equal(t.reshape(-1), sc.indices[: t.size]), "the blob's topology changed with its phase"
    vertices = sc.vertices.copy()
    vertices[: len(v)] = v
    return with_vertices(sc, vertices)


def upload(m, sc):
    """What a host does after a deformation: SetData of the lists that can have changed (equal data dirties nothing)."""
    for buf, data in ((m._meshObjectBuffer, sc.mesh_objects), (m._vertexBuffer, sc.vertices), (m._normalBuffer, sc.normals),
                      (m._meshObjectBVHBuffer, sc.mesh_bvh)):
        buf.SetData(data)
    m._frame = 0; m._currentSample = 0


def frame(m):
    m._frame = 0; m._currentSample = 0
    m.OnRenderImage()
    return m._target.GetPixels()


def stats(ctx):
    return ctx.deform_stats(), ctx.refit_stats(), ctx.blas_cache_stats()[1]


def expect_deformed(sc0, sc1):
    """(deformed, renormed) flags of the restatement for the step sc0 -> sc1."""
    spans = D.vertex_spans(sc0.mesh_objects, sc0.indices)
    return D.meets(spans, D.dirty_range(sc0.vertices, sc1.vertices)), D.meets(spans, D.dirty_range(sc0.normals, sc1.normals))


def check_deform(ctx, other, m, builder, cur, nxt, nodes, tri, root, what, oracle=True):
    """One deformation step through whole-array SetData: counts, nodes against the restatement, frames.  -> the read-back nodes."""
    deformed, renormed = expect_deformed(cur, nxt)
    moved = R.moved_meshes(cur, nxt) | deformed
    d0, (r0, p0), built0 = stats(ctx)
    upload(m, nxt)
    got = frame(m)
    d1, (r1, p1), built1 = stats(ctx)
    assert (d1["deformed"] - d0["deformed"], d1["renormed"] - d0["renormed"]) == (int(deformed.sum()), int(renormed.sum())), (what, d0, d1)
    assert (r1 - r0, p1 - p0) == (int(moved.sum()), 1) and d1["forced_rebuilds"] == d0["forced_rebuilds"], (what, r1 - r0, p1 - p0)
    assert builder != 0 or built1 == built0, what                               # the host builder's cache built nothing
    new, tri2, root2, info = ctx.read_scene_blas(len(nxt.mesh_objects))
    assert np.array_equal(tri2, tri) and np.array_equal(root2, root), what
    want, _ = R.refit(nxt, nodes, tri, root, moved)
    diff = (new.view(np.uint32) != want.view(np.uint32)).any(axis=1)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {len(new)} nodes differ from the restatement, first {np.nonzero(diff)[0][:4]}"
    if np.isfinite(nxt.vertices).all():
        assert validate(nxt, new, tri, root) <= info["max_depth"], what         # a valid BVH of the DEFORMED triangles
    assert bits_equal(got, fresh_frame(other, nxt, builder)), f"{what}: frame differs from a from-scratch preparation"
    if oracle:
        assert bits_equal(got, pyoracle.Oracle(nxt).render(mode=0, threads=8)), f"{what}: frame differs from the oracle's literal walk"
    return new


def start(ctx, sc, builder=0, leaf=2, **options):
    ctx.set_option("kernel_mode", 3)
    ctx.set_option("blas_leaf_max", leaf)                  # (process-wide: the second context's preparations follow)
    ctx.set_option("blas_builder", builder)
    for k, v in options.items():
        ctx.set_option(k, v)
    m = RayTraceMaster(ctx, sc)
    m.OnRenderImage()
    return m, ctx.read_scene_blas(len(sc.mesh_objects))[:3]


# ---- 1. a changed phase --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,builder,leaf", [(SMALL, b, l) for b in (0, 1, 3) for l in (1, 2, 8)] + [(DEEP, b, 2) for b in (0, 1, 3)])
def test_changed_phase_is_refitted_in_place(gpu_ctx, other_ctx, size, builder, leaf):
    sc = mixed(size)
    try:
        m, (nodes, tri, root) = start(gpu_ctx, sc, builder, leaf)
        nxt = blob_phase(sc, size, 1.5)
        assert expect_deformed(sc, nxt)[0].tolist() == [True, False, False]
        check_deform(gpu_ctx, other_ctx, m, builder, sc, nxt, nodes, tri, root, f"phase {size} builder {builder} leaf {leaf}")
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        restore(gpu_ctx)


# ---- 2. ten in a row -----------------------------------------------------------------------------------------------------------------
def test_ten_deformations_in_a_row(gpu_ctx, other_ctx):
    sc = mixed()
    try:
        m, (nodes, tri, root) = start(gpu_ctx, sc, 3)
        cur = sc
        for k in range(10):
            nxt = blob_phase(sc, SMALL, 0.4 * (k + 1), bumps=0.12 + 0.02 * k)
            nodes = check_deform(gpu_ctx, other_ctx, m, 3, cur, nxt, nodes, tri, root, f"step {k}", oracle=k in (0, 9))
            cur = nxt
        assert gpu_ctx.counters()["watchdog_trips"] == 0
        m.OnDisable()
    finally:
        restore(gpu_ctx)


# ---- 3. the single-leaf quad alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 3])
def test_the_quad_alone_is_deformed(gpu_ctx, other_ctx, builder):
    sc = mixed()
    try:
        m, (nodes, tri, root) = start(gpu_ctx, sc, builder)
        v = sc.vertices.copy()
        v[-4:] += np.array([[0.2, 0.3, 0.0], [0.0, -0.2, 0.1], [0.3, 0.1, 0.0], [0.0, 0.0, -0.4]], F)      # no longer planar
        nxt = with_vertices(sc, v)
        assert expect_deformed(sc, nxt)[0].tolist() == [False, False, True]
        check_deform(gpu_ctx, other_ctx, m, builder, sc, nxt, nodes, tri, root, "quad")
        m.OnDisable()
    finally:
        restore(gpu_ctx)


# ---- 4. normals only -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 3])
def test_normals_only(gpu_ctx, other_ctx, builder):
    sc = mixed()
    try:
        m, (nodes, tri, root) = start(gpu_ctx, sc, builder)
        n = sc.normals.copy()
        a, b = N_BLOB[(12, 9)], N_BLOB[(12, 9)] + 42                              # the icosphere's normals, turned and no longer unit
        n[a:b] = (n[a:b] @ np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]], F).T * F(1.25)).astype(F)
        nxt = with_vertices(sc, sc.vertices, normals=n)
        assert not expect_deformed(sc, nxt)[0].any() and expect_deformed(sc, nxt)[1].tolist() == [False, True, False]
        d0, (r0, p0), _ = stats(gpu_ctx)
        upload(m, nxt)
        got = frame(m)
        d1, (r1, p1), _ = stats(gpu_ctx)
        assert (d1["deformed"] - d0["deformed"], d1["renormed"] - d0["renormed"], r1 - r0, p1 - p0) == (0, 1, 0, 1)      # no boxes refitted
        assert d1["bytes_copied"] - d0["bytes_copied"] == 42 * 12
        new = gpu_ctx.read_scene_blas(3)[0]
        assert bits_equal(new, nodes)                                            # no node was touched
        assert bits_equal(got, fresh_frame(other_ctx, nxt, builder))
        assert bits_equal(got, pyoracle.Oracle(nxt).render(mode=0, threads=8))
        mine = gpu_ctx.render_aov_arrays(96, 64)
        f = RayTraceMaster(other_ctx, nxt)
        f.OnRenderImage()                                                        # (binds the scene and the camera for the feature buffers)
        theirs = other_ctx.render_aov_arrays(96, 64)
        f.OnDisable()
        for key in mine:
            assert bits_equal(np.ascontiguousarray(mine[key]).view(F), np.ascontiguousarray(theirs[key]).view(F)), key
        assert ((mine["kind"] == 3) & (mine["object"] == 1)).any()                                       # the icosphere is in view: its normals were compared
        m.OnDisable()
    finally:
        restore(gpu_ctx)


# ---- 5. a deformation and a matrix move in one update ------------------------------------------------------------------------------
@pytest.mark.parametrize("same_mesh", [False, True])
def test_deformation_and_matrix_move_in_one_update(gpu_ctx, other_ctx, same_mesh):
    sc = mixed()
    try:
        m, (nodes, tri, root) = start(gpu_ctx, sc, 0)
        nxt = blob_phase(sc, SMALL, 2.2)
        k = 0 if same_mesh else 1
        nxt = moved_scene(nxt, {k: scenes.trs(translate=(-1.5, 1.6, 0.4) if same_mesh else (2.0, 1.4, -0.5), scale=(1.1, 0.8, 1.3), yaw_deg=-40.0)})
        assert int((R.moved_meshes(sc, nxt) | expect_deformed(sc, nxt)[0]).sum()) == (1 if same_mesh else 2)
        check_deform(gpu_ctx, other_ctx, m, 0, sc, nxt, nodes, tri, root, f"deform + move, same mesh {same_mesh}")
        m.OnDisable()
    finally:
        restore(gpu_ctx)


# ---- 6. ranged SetData ---------------------------------------------------------------------------------------------------------------
def test_ranged_set_data_of_single_vertices(gpu_ctx, other_ctx):
    sc = mixed()
    nb = N_BLOB[(12, 9)]
    try:
        m, (nodes, tri, root) = start(gpu_ctx, sc, 3)
        # one vertex of the icosphere: only that mesh is refitted, 12 bytes are copied, and the result is that of a whole-array SetData
        v = sc.vertices.copy(); v[nb + 5] *= F(1.3)
        nxt = with_vertices(sc, v, recompute=False)
        d0, (r0, p0), _ = stats(gpu_ctx)
        m._vertexBuffer.SetData(v, nb + 5, nb + 5, 1)
        m._meshObjectBVHBuffer.SetData(nxt.mesh_bvh)
        got = frame(m)
        d1, (r1, p1), _ = stats(gpu_ctx)
        assert (d1["deformed"] - d0["deformed"], d1["renormed"] - d0["renormed"], r1 - r0, p1 - p0) == (1, 0, 1, 1)
        assert d1["bytes_copied"] - d0["bytes_copied"] == 12
        new = gpu_ctx.read_scene_blas(3)[0]
        assert bits_equal(new, R.refit(nxt, nodes, tri, root, np.array([False, True, False]))[0])
        assert bits_equal(got, fresh_frame(other_ctx, nxt, 3))
        m2, _ = start(other_ctx, sc, 3, refit=1)                                 # the same change through a whole-array SetData
        upload(m2, nxt)
        assert bits_equal(got, frame(m2)) and bits_equal(new, other_ctx.read_scene_blas(3)[0])
        m2.OnDisable(); other_ctx.set_option("refit", 0)
        # two disjoint ranged calls before one frame are united: blob vertex 3 and the quad's last vertex -> everything in between
        v2 = v.copy(); v2[3] *= F(0.9); v2[-1, 1] += F(0.25)
        nxt2 = with_vertices(nxt, v2, recompute=False)
        m._vertexBuffer.SetData(v2[3:4], 0, 3, 1)
        m._vertexBuffer.SetData(v2, len(v2) - 1, len(v2) - 1, 1)
        m._meshObjectBVHBuffer.SetData(nxt2.mesh_bvh)
        got = frame(m)
        d2, (r2, p2), _ = stats(gpu_ctx)
        assert (d2["deformed"] - d1["deformed"], r2 - r1, p2 - p1) == (3, 3, 1)  # conservative: the icosphere lies inside the united range
        assert d2["bytes_copied"] - d1["bytes_copied"] == (len(v2) - 3) * 12
        assert bits_equal(got, fresh_frame(other_ctx, nxt2, 3))
        # equal data: the scene is not stale
        m._vertexBuffer.SetData(v2[10:20], 0, 10, 10)
        m._vertexBuffer.SetData(v2, 0, 0, 0)
        frame(m)
        assert stats(gpu_ctx)[:2] == (d2, (r2, p2))
        # argument errors leave buffer and scene untouched
        lib, h, buf = gpu_ctx.lib, gpu_ctx._h, m._vertexBuffer
        junk = np.full((4, 3), 77.0, F)
        p = junk.ctypes.data_as(C.c_void_p)
        for first, data, count in ((-1, p, 1), (0, p, -1), (len(v2) - 3, p, 4), (len(v2), p, 1), (0, None, 1), (2 ** 31 - 1, p, 2)):
            assert lib.urt_buffer_set_data_range(h, buf.handle, first, data, count) == 1, (first, count)
        assert lib.urt_buffer_set_data_range(h, 0xdead, 0, p, 1) == 2
        assert lib.urt_buffer_set_data_range(h, buf.handle, 0, None, 0) == 0
        with pytest.raises(UrtError):
            buf.SetData(junk, 2, 0, 3)
        assert bits_equal(frame(m), got) and stats(gpu_ctx)[:2] == (d2, (r2, p2))
        assert bits_equal(gpu_ctx.read_scene_blas(3)[0], R.refit(nxt2, new, tri, root, np.array([True, True, True]))[0])
        m.OnDisable()
    finally:
        restore(gpu_ctx)


def test_elements_never_set_read_as_zero(gpu_ctx, other_ctx):
    sc = mixed()
    nb = N_BLOB[(12, 9)]
    try:
        m, _ = start(gpu_ctx, sc, 0)
        buf = ComputeBuffer(gpu_ctx, len(sc.vertices), 12)
        buf.SetData(sc.vertices, nb, nb, len(sc.vertices) - nb)                  # the blob's vertices are never set
        old, m._vertexBuffer = m._vertexBuffer, buf                              # (the next frame binds it: a full preparation)
        zeroed = sc.vertices.copy(); zeroed[:nb] = 0
        assert bits_equal(frame(m), fresh_frame(other_ctx, with_vertices(sc, zeroed, recompute=False, heap=False), 0))
        old.Release()
        m.OnDisable()
    finally:
        restore(gpu_ctx)


# ---- 7. changes that fall back to a full preparation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["indices", "count", "refit0", "refit_vertices0"])
def test_fallbacks_prepare_from_scratch(gpu_ctx, case):
    sc = mixed()
    try:
        m, _ = start(gpu_ctx, sc, 0)
        nxt = blob_phase(sc, SMALL, 0.9)
        if case == "refit0":
            gpu_ctx.set_option("refit", 0)
            m.OnRenderImage()
        if case == "refit_vertices0":
            gpu_ctx.set_option("refit_vertices", 0)
        d0, (r0, p0), built0 = stats(gpu_ctx)
        if case == "indices":
            nxt = copy.copy(nxt)
            i = nxt.indices.copy(); i[:3] = i[[1, 2, 0]]                           # the same triangle, another first vertex
            nxt.indices = i
            m._indexBuffer.SetData(nxt.indices)
        if case == "count":                                                       # a vertex buffer of another count, rebound
            nxt = copy.copy(nxt)
            nxt.vertices = np.concatenate([nxt.vertices, np.zeros((3, 3), F)])
            nxt.normals = np.concatenate([nxt.normals, np.zeros((3, 3), F)])
            m._vertexBuffer = m.CreateComputeBuffer(m._vertexBuffer, nxt.vertices, 12)
            m._normalBuffer = m.CreateComputeBuffer(m._normalBuffer, nxt.normals, 12)
        upload(m, nxt)
        got = frame(m)
        d1, (r1, p1), built1 = stats(gpu_ctx)
        assert d1 == d0 and (r1, p1) == (r0, p0), case                           # nothing in place
        assert built1 == built0 + 1, case                                        # the host cache rebuilt the blob alone
        o = pyoracle.Oracle(nxt)
        assert bits_equal(got, o.render(mode=0, threads=8)), case
        m.OnDisable()
    finally:
        restore(gpu_ctx)


# ---- 8. non-finite, collapsed and far-away vertices, and back -------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 3])
def test_extreme_vertices_and_back(gpu_ctx, other_ctx, builder):
    sc = mixed()
    nb = N_BLOB[(12, 9)]
    try:
        m, (nodes, tri, root) = start(gpu_ctx, sc, builder)
        steps = []
        v = sc.vertices.copy(); v[5] = np.nan; v[17, 1] = np.inf; v[40] = (-np.inf, 0.0, np.nan); steps.append(("nan / inf", v))
        v = sc.vertices.copy(); v[nb: nb + 42] = v[nb]; steps.append(("collapsed to a point", v))
        v = sc.vertices.copy(); v[:nb] += F(1e5); steps.append(("1e5 away", v))
        steps.append(("back", sc.vertices.copy()))
        cur = sc
        for what, v in steps:
            nxt = with_vertices(sc, v, recompute=False, heap=bool(np.isfinite(v).all()))      # (a heap cannot be built from NaN bounds)
            nodes = check_deform(gpu_ctx, other_ctx, m, builder, cur, nxt, nodes, tri, root, f"{what} builder {builder}")
            cur = nxt
        assert gpu_ctx.counters()["watchdog_trips"] == 0
        m.OnDisable()
    finally:
        restore(gpu_ctx)


# ---- 9. deferred frames --------------------------------------------------------------------------------------------------------------
def test_deformation_inside_deferred_frames(gpu_ctx):
    sc = mixed()
    nxt = blob_phase(sc, SMALL, 1.1)

    def protocol(fpl, refit):
        gpu_ctx.set_option("frames_per_launch", fpl); gpu_ctx.set_option("refit", refit)
        m = RayTraceMaster(gpu_ctx, sc)
        for _ in range(3):
            m.OnRenderImage()                                                    # dispatched before the deformation: the old shape
        d0 = gpu_ctx.deform_stats()["deformed"]
        for buf, data in ((m._vertexBuffer, nxt.vertices), (m._normalBuffer, nxt.normals), (m._meshObjectBVHBuffer, nxt.mesh_bvh)):
            buf.SetData(data)
        for _ in range(3):
            m.OnRenderImage()
        out = m._converged.GetPixels()
        n = gpu_ctx.deform_stats()["deformed"] - d0
        m.OnDisable()
        return out, n

    try:
        a, na = protocol(4, 1)
        b, nb = protocol(1, 0)
        assert (na, nb) == (1, 0) and bits_equal(a, b)
    finally:
        restore(gpu_ctx)


# ---- 10. derived copies --------------------------------------------------------------------------------------------------------------
def test_derived_copies_follow_the_deformation(gpu_ctx, other_ctx):
    sc = mixed(DEEP)
    nxt = blob_phase(sc, DEEP, 1.9)
    try:
        # quantized nodes
        m, _ = start(gpu_ctx, sc, 3, qnodes=1)
        upload(m, nxt)
        got = frame(m)
        assert gpu_ctx.read_scene_qnodes()[2] and gpu_ctx.deform_stats()["cost_ratio"] > 0
        other_ctx.set_option("qnodes", 1)
        assert bits_equal(got, fresh_frame(other_ctx, nxt, 3))
        other_ctx.set_option("qnodes", 0)
        assert bits_equal(got, fresh_frame(other_ctx, nxt, 3))
        m.OnDisable()
        gpu_ctx.set_option("qnodes", 0)
        # normal cones: the words meet the obligation on the deformed triangle records, which are the restatement's
        m, (nodes, tri, root) = start(gpu_ctx, sc, 3, blas_cones=1)
        w0 = gpu_ctx.read_scene_cones()[0]
        d0 = gpu_ctx.deform_stats()["deformed"]
        upload(m, nxt)
        got = frame(m)
        assert gpu_ctx.deform_stats()["deformed"] == d0 + 1
        words, e1, e2, in_use = gpu_ctx.read_scene_cones()
        rec = R.records(nxt, tri)
        assert in_use and bits_equal(e1, rec["e1"]) and bits_equal(e2, rec["e2"]) and (words != w0).any()
        first, count = K.child_ranges(nodes, root)
        d = np.random.default_rng(5).normal(size=(1000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        n_skips, n_cones = K.check_obligation(words, first, count, e1, e2, d)
        assert n_cones > 0 and n_skips > 0, (n_cones, n_skips)
        assert bits_equal(got, fresh_frame(other_ctx, nxt, 3))
        # ray queries at deformed vertices and the feature buffers, against a fresh context
        verts = R.reconstructed(rec)[::37, 0].astype(np.float64)
        o = verts + np.array([0.3, 2.5, -4.0])
        O, Dr = o.astype(F), (verts - o).astype(F)
        mine_hits, mine_aov = gpu_ctx.ray_query(O, Dr), gpu_ctx.render_aov_arrays(160, 104)
        f = RayTraceMaster(other_ctx, nxt)
        f.OnRenderImage()
        their_hits, their_aov = other_ctx.ray_query(O, Dr), other_ctx.render_aov_arrays(160, 104)
        f.OnDisable()
        assert mine_hits.tobytes() == their_hits.tobytes() and (mine_hits["kind"] != 0).sum() > len(O) // 2
        for key in mine_aov:
            assert bits_equal(np.ascontiguousarray(mine_aov[key]).view(F), np.ascontiguousarray(their_aov[key]).view(F)), key
        m.OnDisable()
    finally:
        other_ctx.set_option("qnodes", 0)
        restore(gpu_ctx)


# ---- 11. cost ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,builder", [(SMALL, 0), (SMALL, 3), (DEEP, 0), (DEEP, 1)])
def test_scene_cost_agrees_with_the_restatement(gpu_ctx, size, builder):
    """Within terms x 2^-23 relative: the worst case of summing the non-negative terms in float32 in any order."""
    sc = mixed(size)
    try:
        m, (nodes, tri, root) = start(gpu_ctx, sc, builder)

        def check(nodes, base_nodes, what):
            got = gpu_ctx.scene_cost(3)
            for col, nd in ((0, nodes), (1, base_nodes)):
                want, terms = D.tree_cost(nd, root)
                err = np.abs(got[:, col].astype(np.float64) - want)
                print(f"{what} {size[1]} builder {builder} col {col}: cost {got[:, col]}, restatement {want}, terms {terms}, rel err {err / np.maximum(want, 1e-300)}")
                assert (err <= terms * 2.0 ** -23 * want).all(), (what, col, got[:, col], want)
            return got

        got = check(nodes, nodes, "built")
        assert got[0, 0] > 1 and got[1, 0] > 1 and got[2, 0] == 0 and np.array_equal(got[:, 0], got[:, 1])
        upload(m, blob_phase(sc, size, 2.6, bumps=0.3))
        new = gpu_ctx.read_scene_blas(3)[0]
        got = check(new, nodes, "deformed")
        ratio = gpu_ctx.deform_stats()["cost_ratio"]
        assert ratio == F(got[0, 0]) / F(got[0, 1]) and got[0, 0] != got[0, 1] and got[1, 0] == got[1, 1]
        m.OnDisable()
    finally:
        restore(gpu_ctx)


# ---- 12. policy ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pct", [101, 0])
def test_a_spoilt_tree_is_rebuilt_when_asked(gpu_ctx, other_ctx, pct):
    sc = mixed(DEEP)
    nb = N_BLOB[(40, 31)]
    try:
        m, (nodes, tri, root) = start(gpu_ctx, sc, 0, refit_rebuild_pct=pct)
        v = sc.vertices.copy()
        v[:nb] = v[:nb][np.random.default_rng(12).permutation(nb)]                # a valid mesh, a useless topology
        nxt = with_vertices(sc, v)
        base = D.tree_cost(nodes, root)[0]
        spoilt = D.tree_cost(R.refit(nxt, nodes, tri, root, np.array([True, False, False]))[0], root)[0]
        assert spoilt[0] >= 2 * base[0], (spoilt, base)
        d0, (r0, p0), _ = stats(gpu_ctx)
        upload(m, nxt)
        got = frame(m)
        d1, (r1, p1), _ = stats(gpu_ctx)
        if pct:
            assert d1["forced_rebuilds"] == d0["forced_rebuilds"] + 1 and (r1, p1) == (r0, p0) and d1["deformed"] == d0["deformed"]
            cost = gpu_ctx.scene_cost(3)
            assert np.array_equal(cost[:, 0], cost[:, 1])                        # a new tree, a new baseline
        else:
            assert d1["forced_rebuilds"] == d0["forced_rebuilds"] and (r1 - r0, p1 - p0) == (1, 1) and d1["deformed"] == d0["deformed"] + 1
        assert d1["cost_ratio"] >= 2.0 * (1 - 1e-5)
        assert bits_equal(got, pyoracle.Oracle(nxt).render(mode=0, threads=8))
        assert bits_equal(got, fresh_frame(other_ctx, nxt, 0))
        m.OnDisable()
    finally:
        restore(gpu_ctx)


def test_rebuild_pct_range(gpu_ctx):
    for bad in (-1, 1, 100):
        with pytest.raises(UrtError):
            gpu_ctx.set_option("refit_rebuild_pct", bad)
    gpu_ctx.set_option("refit_rebuild_pct", 101)
    gpu_ctx.set_option("refit_rebuild_pct", 0)


# ---- many meshes at once -------------------------------------------------------------------------------------------------------------
def test_many_meshes_deformed_at_once(gpu_ctx, other_ctx):
    sc = scenes.many_meshes_scene(128, 80, n=128, level=1)
    try:
        m, (nodes, tri, root) = start(gpu_ctx, sc, 3)
        v = sc.vertices.copy()
        per = len(v) // 128
        rng = np.random.default_rng(3)
        for k in range(0, 128, 2):                                               # every other mesh, its own squash
            v[k * per: (k + 1) * per] *= rng.uniform(0.7, 1.3, 3).astype(F)
        nxt = with_vertices(sc, v)
        # the dirty range spans the meshes in between: conservative, they are refitted to the boxes they had
        assert expect_deformed(sc, nxt)[0].sum() == 127
        check_deform(gpu_ctx, other_ctx, m, 3, sc, nxt, nodes, tri, root, "128 meshes", oracle=False)
        m.OnDisable()
    finally:
        restore(gpu_ctx)


# ---- 13. DeformMeshes ----------------------------------------------------------------------------------------------------------------
def test_deform_meshes_with_and_without_temporal_accumulation(gpu_ctx, other_ctx):
    sc = mixed()
    v_new = scenes.uv_blob(12, 9, phase=1.3)[0]
    try:
        m = RayTraceMaster(gpu_ctx, copy.copy(sc))
        m.EnableTemporalAccumulation()
        for _ in range(6):
            m.OnRenderImage()
        d0 = gpu_ctx.deform_stats()["deformed"]
        m.DeformMeshes({0: v_new})
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
        nxt = blob_phase(sc, SMALL, 1.3)
        assert bits_equal(np.asarray(m.scene.vertices), nxt.vertices) and bits_equal(np.asarray(m.scene.normals), host_normals(nxt))
        m.OnDisable()
        # temporal accumulation off: the mean restarts, and the frame is that of the deformed scene
        m = RayTraceMaster(gpu_ctx, copy.copy(sc))
        for _ in range(3):
            m.OnRenderImage()
        m.DeformMeshes({0: v_new}, recompute_normals=False)
        assert m._currentSample == 0
        m._frame = 0
        m.OnRenderImage()
        assert bits_equal(m._target.GetPixels(), fresh_frame(other_ctx, with_vertices(sc, nxt.vertices, recompute=False), -1))
        m.OnDisable()
    finally:
        restore(gpu_ctx)


def host_normals(sc):
    from unityraytracer_amd import host_scene
    return host_scene.compute_normals(sc.vertices, sc.indices)



# ---- 14. resources -------------------------------------------------------------------------------------------------------------------
def test_resources_return_to_the_baseline(gpu_ctx):
    gpu_ctx.synchronize()
    base = live_resources()
    sc = mixed()
    for builder in (0, 3):
        with Context(gpu_ctx.device) as ctx:
            m, _ = start(ctx, sc, builder)
            upload(m, blob_phase(sc, SMALL, 0.8))
            frame(m)
            n = sc.normals.copy(); n[:5] *= F(2)
            upload(m, with_vertices(sc, blob_phase(sc, SMALL, 0.8).vertices, normals=n))
            frame(m)
            s = ctx.deform_stats()
            assert s["deformed"] == 1 and s["renormed"] >= 1 and live_resources()["device_bytes"] > base["device_bytes"]
            m.OnDisable()
    gpu_ctx.set_option("blas_leaf_max", 2)
    assert live_resources() == base
