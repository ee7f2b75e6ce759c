"""GPU: blend shapes on the device (include/urt.h urt_morph_plan_create, urt_morph_vertices; csrc/morph.hip) and
RayTraceMaster.AttachBlendShapes / MorphMeshes on top of them.  The kernel is held to the numpy restatement of tests/morph_ref.py bit for
bit (a NaN equals a NaN); the chain morph -> skin -> normals is held to the restatements chained the same way; frames after MorphMeshes
are held, bit for bit, to a from-scratch preparation of the restated vertices and normals on a second context and to the oracle's
literal walk, and the counters show that the positions never touched the host."""
import copy
import ctypes as C

import numpy as np
import pytest

import morph_ref as M
import skin_ref as S
from test_gpu_deform import N_BLOB, SMALL, frame, mixed, other_ctx, restore, start, stats, with_vertices  # noqa: F401  (other_ctx: a fixture)
from test_gpu_reproject_deform import near_scene, started
from test_gpu_skin import check_skinned_frame, f32, same
from unityraytracer_amd import ComputeBuffer, Context, _lib, host_scene, live_resources

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = F(7.5)
INVALID_ARGUMENT, INVALID_HANDLE, SCENE = 1, 2, 8


class RawMorph:
    """A plan, its rest buffers, a weight table and two destinations filled with a sentinel, all 12-byte buffers of `n` elements."""

    def __init__(self, ctx, rest_v, rest_n, deltas, weights, first, count):
        n = len(rest_v)
        self.ctx, self.n = ctx, n
        self.plan = ctx.morph_plan(deltas, len(weights), first, count)
        self.rest_v, self.rest_n = ComputeBuffer(ctx, n, 12), ComputeBuffer(ctx, n, 12)
        self.weights = ComputeBuffer(ctx, len(weights), 4)
        self.dst_v, self.dst_n = ComputeBuffer(ctx, n, 12), ComputeBuffer(ctx, n, 12)
        for b, a in ((self.rest_v, rest_v), (self.rest_n, rest_n), (self.weights, weights)):
            b.SetData(np.ascontiguousarray(a))
        self.reset()

    def reset(self):
        for b in (self.dst_v, self.dst_n):
            b.SetData(np.full((self.n, 3), SENTINEL, F))

    def morph(self, normals=True, normalize=False):
        self.plan.morph(self.rest_v, self.rest_n if normals else None, self.weights, self.dst_v, self.dst_n if normals else None, normalize)

    def all(self):
        return (self.rest_v, self.rest_n, self.weights, self.dst_v, self.dst_n)

    def release(self):
        self.plan.Release()
        for b in self.all():
            b.Release()


def variant_case(variant, first, count, n_targets, seed):
    """(rest positions, rest normals, deltas, weights) of first + count + 3 vertices, of which first .. first + count - 1 are served."""
    rng = np.random.default_rng(seed)
    n = first + count + 3
    P = rng.uniform(-3, 3, (n, 3)).astype(F)
    N = rng.normal(size=(n, 3)).astype(F)
    touched = rng.random((n_targets, count)) < min(0.6, 6.0 / n_targets)          # about six entries a vertex at most
    target, vertex = np.nonzero(touched)
    mix = rng.permutation(len(vertex))                                            # the input comes in no order
    vertex, target = first + vertex[mix], target[mix]
    dp, dn = rng.uniform(-1, 1, (len(vertex), 3)).astype(F), rng.uniform(-1, 1, (len(vertex), 3)).astype(F)
    w = rng.uniform(-1, 1.5, n_targets).astype(F)
    w[w == 0] = 1
    if variant == "mostly_zero":                             # a handful of live targets; the dead ones carry inf and NaN deltas
        dead = rng.random(n_targets) < 0.85
        dead[0] = True
        w[dead] = 0
        w[-1] = F(-0.0) if n_targets > 1 else w[-1]
        on_dead = w[target] == 0
        wild = rng.choice(np.array([np.inf, -np.inf, np.nan, 3e38], F), (len(vertex), 3))
        dp[on_dead], dn[on_dead] = wild[on_dead], wild[on_dead][:, ::-1]
    elif variant == "nan_weight":
        w[n_targets // 2] = np.nan
    elif variant == "negative_huge":
        w = rng.choice(np.array([-2.5, -1e-30, 1e30, -3e38, 3.4e38, 0.5], F), n_targets)
    elif variant == "duplicates":                            # the same (vertex, target) pair again and again, apart in the input
        if len(vertex):
            again = rng.integers(0, len(vertex), 3 * count + 5)
            vertex, target = np.concatenate([vertex, vertex[again]]), np.concatenate([target, target[again]])
            dp = np.concatenate([dp, rng.uniform(-1, 1, (len(again), 3)).astype(F)])
            dn = np.concatenate([dn, rng.uniform(-1, 1, (len(again), 3)).astype(F)])
    elif variant == "valence":                               # valence 0 and valence 100 next to each other in one wave
        heavy = first + min(1, count - 1)
        keep = (vertex != heavy) & ((vertex != first) | (count == 1))
        vertex, target, dp, dn = vertex[keep], target[keep], dp[keep], dn[keep]
        vertex = np.concatenate([np.full(50, heavy), vertex, np.full(50, heavy)])
        target = np.concatenate([rng.integers(0, n_targets, 50), target, rng.integers(0, n_targets, 50)])
        dp = np.concatenate([rng.uniform(-1, 1, (50, 3)).astype(F), dp, rng.uniform(-1, 1, (50, 3)).astype(F)])
        dn = np.concatenate([rng.uniform(-1, 1, (50, 3)).astype(F), dn, rng.uniform(-1, 1, (50, 3)).astype(F)])
    elif variant == "negzero":                               # -0.0 in the rest pose under entries that are all dead
        w[:] = 0
        w[::2] = F(-0.0)
        P[first: first + count: 2, 0] = F(-0.0)
        P[first, :] = F(-0.0)
        N[first: first + count: 3, 2] = F(-0.0)
    else:
        assert variant == "plain"
    return P, N, M.deltas_array(vertex, target, dp, dn), w


VARIANTS = ("plain", "mostly_zero", "nan_weight", "negative_huge", "duplicates", "valence", "negzero")
MODES = ((False, False), (True, False), (True, True))          # (normals, normalize)


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_targets", [1, 3, 300])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, 1202])
def test_morph_vertices_equals_the_restatement(gpu_ctx, count, n_targets):
    assert 257 > M.BLOCK and 1202 > 4 * M.BLOCK              # more than one workgroup, and a ragged last one
    for vi, variant in enumerate(VARIANTS):
        for first in (0, 5):
            n = first + count + 3
            P, N, d, w = variant_case(variant, first, count, n_targets, seed=1000 * vi + 7 * count + first + n_targets)
            raw = RawMorph(gpu_ctx, P, N, d, w, first, count)
            ranges, _, (n_entries, max_valence, n_touched) = M.plan(d, first, count)
            info = raw.plan.info()
            assert {k: info[k] for k in ("first", "count", "n_targets", "n_entries", "max_valence", "n_touched")} == \
                {"first": first, "count": count, "n_targets": n_targets, "n_entries": n_entries, "max_valence": max_valence, "n_touched": n_touched}
            assert info["device_bytes"] == 8 * count + 28 * n_entries
            if variant == "valence":
                assert max_valence == 100 and (count == 1 or ranges[0, 1] == 0)
            for normals, normalize in MODES:
                want_v, want_n = M.morph(P, N if normals else None, d, first, count, w, normalize)
                raw.reset()
                written = (raw.dst_v, raw.dst_n) if normals else (raw.dst_v,)
                downloads = [gpu_ctx.buffer_state(buf)["downloads"] for buf in written]
                raw.morph(normals, normalize)
                for buf, dl in zip(written, downloads):      # stale as a whole, and nothing came back before the read below
                    state = gpu_ctx.buffer_state(buf)
                    assert (state["stale_first"], state["stale_last"], state["mirror_bytes"], state["downloads"]) == (first, first + count - 1, n * 12, dl)
                got_v, got_n = f32(raw.dst_v), f32(raw.dst_n)
                what = (variant, first, count, n_targets, normals, normalize)
                inside = slice(first, first + count)
                assert same(got_v[inside], want_v), what
                assert same(got_n[inside], want_n if normals else np.full((count, 3), SENTINEL, F)), what
                outside = np.ones(n, bool); outside[inside] = False
                assert (got_v[outside] == SENTINEL).all() and (got_n[outside] == SENTINEL).all(), what
                if variant == "negzero":                     # no live entry: the rest position bit for bit, -0.0 included
                    assert got_v[inside].tobytes() == P[inside].tobytes() and np.signbit(got_v[first]).all(), what
                    if normals and not normalize:
                        assert got_n[inside].tobytes() == N[inside].tobytes(), what
            raw.release()


def test_an_empty_plan_and_a_plan_without_deltas(gpu_ctx):
    P, N, d, w = variant_case("plain", 2, 9, 3, seed=3)
    raw = RawMorph(gpu_ctx, P, N, d[:0], w, 2, 9)            # no deltas: the rest pose is copied
    raw.morph()
    assert f32(raw.dst_v)[2:11].tobytes() == P[2:11].tobytes() and f32(raw.dst_n)[2:11].tobytes() == N[2:11].tobytes()
    assert (f32(raw.dst_v)[:2] == SENTINEL).all() and (f32(raw.dst_v)[11:] == SENTINEL).all() and raw.plan.info()["n_entries"] == 0
    empty = gpu_ctx.morph_plan(d[:0], 3, 4, 0)               # nothing served: OK after the checks, nothing marked
    raw.reset()
    before = [gpu_ctx.buffer_state(b) for b in raw.all()]
    empty.morph(raw.rest_v, raw.rest_n, raw.weights, raw.dst_v, raw.dst_n)
    assert [gpu_ctx.buffer_state(b) for b in raw.all()] == before and empty.info()["device_bytes"] == 0
    with pytest.raises(_lib.UrtError) as e:
        empty.morph(raw.rest_v, raw.rest_n, raw.weights, raw.rest_v, raw.dst_n)
    assert e.value.code == INVALID_ARGUMENT
    empty.Release(); raw.release()


# ---- 2. the chain: blend shapes, then bones, then normals ---------------------------------------------------------------------------
def blob_shapes(sc, nb, seed=4):
    """Three blend shapes of the blob, dense as Mesh.GetBlendShapeFrameVertices returns them: an inflation along the normals, a shear
    that touches the upper half only, and a target without normal deltas that moves every third vertex."""
    rng = np.random.default_rng(seed)
    v, nrm = sc.vertices[:nb], sc.normals[:nb]
    inflate = (F(0.15) * nrm).astype(F)
    shear = np.zeros((nb, 3), F)
    upper = v[:, 1] > v[:, 1].mean()
    shear[upper, 0] = F(0.3) * (v[upper, 1] - v[:, 1].mean())
    tilt = np.zeros((nb, 3), F)
    tilt[upper, 1] = F(0.2)
    jitter = np.zeros((nb, 3), F)
    jitter[::3] = rng.uniform(-0.05, 0.05, (len(jitter[::3]), 3)).astype(F)
    return [(inflate, (F(0.1) * nrm).astype(F)), (shear, tilt), (jitter, None)]


def shapes_as_deltas(targets, first):
    """The urt_MorphDeltas AttachBlendShapes makes of dense targets: rows whose six deltas are all zero dropped, absolute vertex numbers."""
    parts = []
    for t, (dp, dn) in enumerate(targets):
        dn = np.zeros_like(dp) if dn is None else dn
        rows = np.flatnonzero((dp != 0).any(axis=1) | (dn != 0).any(axis=1))
        parts.append(M.deltas_array(first + rows, np.full(len(rows), t), dp[rows], dn[rows]))
    return np.concatenate(parts)


def test_morph_then_skin_then_normals_equals_the_restatements_chained(gpu_ctx):
    sc = mixed()
    nb = N_BLOB[SMALL[1]]
    first, n = 4, nb + 9                                      # the blob as elements 4 .. of larger buffers
    P, N = np.full((n, 3), 2.5, F), np.full((n, 3), 0.5, F)
    P[first: first + nb], N[first: first + nb] = sc.vertices[:nb], sc.normals[:nb]
    assert int(sc.mesh_objects[0]["indices_offset"]) == 0
    tris = (sc.indices[: int(sc.mesh_objects[0]["indices_count"])] + first).astype(np.int32)
    assert tris.min() == first and tris.max() == first + nb - 1
    d = shapes_as_deltas(blob_shapes(sc, nb), first)
    idx, wgt = np.zeros((n, 4), np.int32), np.zeros((n, 4), F)
    idx[first: first + nb], wgt[first: first + nb], _ = S.two_bone_bend(sc.vertices[:nb], 30.0)
    ctx = gpu_ctx
    raw = RawMorph(ctx, P, N, d, np.zeros(3, F), first, nb)   # dst_v / dst_n: the intermediates
    ib, wb, bones_b = ComputeBuffer(ctx, n, 16), ComputeBuffer(ctx, n, 16), ComputeBuffer(ctx, 2, 48)
    out_v, out_n, tri_b = ComputeBuffer(ctx, n, 12), ComputeBuffer(ctx, n, 12), ComputeBuffer(ctx, len(tris), 4)
    ib.SetData(idx); wb.SetData(wgt); tri_b.SetData(tris)
    out_v.SetData(P); out_n.SetData(np.full((n, 3), SENTINEL, F))
    nplan = ctx.normals_plan(out_v, tri_b, first, nb)        # the topology of the rest pose: no deformation below welds or splits anything
    for step, (w, angle) in enumerate(((np.array([1.0, 0.5, 1.0], F), 30.0), (np.array([0.0, -0.7, 0.0], F), -20.0))):
        bones = S.two_bone_bend(sc.vertices[:nb], angle)[2]
        raw.weights.SetData(w); bones_b.SetData(bones)
        chain = (raw.dst_v, raw.dst_n, out_v, out_n)
        downloads = [ctx.buffer_state(buf)["downloads"] for buf in chain]
        raw.morph()
        ctx.skin_vertices(raw.dst_v, raw.dst_n, ib, wb, bones_b, first, nb, out_v, out_n)
        mid_v, mid_n = M.morph(P, N, d, first, nb, w)
        want_v, want_n = S.skin(mid_v, mid_n, idx[first: first + nb], wgt[first: first + nb], bones)
        # nothing came back: the skin read the morph's result where it was written
        assert [ctx.buffer_state(buf)["downloads"] for buf in chain] == downloads, step
        assert same(f32(out_v)[first: first + nb], want_v) and same(f32(out_n)[first: first + nb], want_n), step
        assert same(f32(raw.dst_v)[first: first + nb], mid_v) and same(f32(raw.dst_n)[first: first + nb], mid_n), step
        assert not same(mid_v, P[first: first + nb]) and not same(want_v, mid_v)
        # the same again, and the normals from the skinned positions instead
        raw.morph()
        ctx.skin_vertices(raw.dst_v, None, ib, wb, bones_b, first, nb, out_v, None)
        nplan.compute(out_n)
        full = P.copy()
        full[first: first + nb] = want_v
        with np.errstate(all="ignore"):
            want_n2 = host_scene.compute_normals(full, tris)
        got_n = f32(out_n)
        assert same(got_n[first: first + nb], want_n2[first: first + nb]), step
        assert (got_n[:first] == SENTINEL).all() and (got_n[first + nb:] == SENTINEL).all()
        assert same(f32(out_v)[first: first + nb], want_v) and (f32(out_v)[:first] == 2.5).all()
    nplan.Release(); raw.release()
    for b in (ib, wb, bones_b, out_v, out_n, tri_b):
        b.Release()


def morphed_scene(sc, nb, targets, w, heap, skin=None):
    """The scene the restatements make of MorphMeshes: the blob morphed (normalised normals), or morphed and then skinned."""
    d = shapes_as_deltas(targets, 0)
    if skin is None:
        v, nrm = M.morph(sc.vertices, sc.normals, d, 0, nb, w, normalize=True)
    else:
        v, nrm = S.skin(*M.morph(sc.vertices, sc.normals, d, 0, nb, w), *skin)
    vertices, normals = sc.vertices.copy(), sc.normals.copy()
    vertices[:nb], normals[:nb] = v, nrm
    out = with_vertices(sc, vertices, normals=normals, heap=False)
    out.mesh_bvh = heap
    return out


@pytest.mark.parametrize("builder", [0, 3])
def test_morphed_frames(gpu_ctx, other_ctx, builder):
    sc = mixed()
    nb = N_BLOB[SMALL[1]]
    targets = blob_shapes(sc, nb)
    idx, wgt, _ = S.two_bone_bend(sc.vertices[:nb], 10.0)
    try:
        m, (nodes, tri, root) = start(gpu_ctx, copy.copy(sc), builder, 2)
        m.AttachBlendShapes(0, targets)
        m.AttachSkin(0, idx, wgt)
        steps = ((np.array([1.0, 0.5, 1.0], F), None), (np.array([0.3, -0.8, 0.0], F), 35.0), (np.array([0.0, 0.0, 0.0], F), None),
                 (np.array([-0.5, 1.0, 2.0], F), -20.0))
        for step, (w, angle) in enumerate(steps):
            bones = None if angle is None else S.two_bone_bend(sc.vertices[:nb], angle)[2]
            d0, (r0, p0), built0 = stats(gpu_ctx)
            m.MorphMeshes({0: w}, poses=None if bones is None else {0: bones})
            assert m._currentSample == 0
            nxt = morphed_scene(sc, nb, targets, w, m.scene.mesh_bvh, None if bones is None else (idx, wgt, bones))
            if step < 2:
                assert not same(nxt.vertices[:nb], sc.vertices[:nb])
            nodes = check_skinned_frame(gpu_ctx, other_ctx, m, builder, sc, nxt, nodes, tri, root, f"builder {builder} step {step}", oracle=step < 2)
            d1, (r1, p1), built1 = stats(gpu_ctx)
            assert (d1["deformed"] - d0["deformed"], d1["renormed"] - d0["renormed"], r1 - r0, p1 - p0) == (1, 1, 1, 1), (d0, d1)
            assert d1["bytes_copied"] - d0["bytes_copied"] == 2 * nb * 12 and d1["forced_rebuilds"] == d0["forced_rebuilds"]
            bufs = (m._vertexBuffer, m._normalBuffer) + (tuple(m._morphBuffers[2:]) if bones is not None else ())
            for buf in bufs:                                 # neither the positions nor the morphed rest pose touched the host
                st = gpu_ctx.buffer_state(buf)
                assert st["downloads"] == 0 and (st["stale_first"], st["stale_last"]) == (0, nb - 1), st
        assert m._morphs[0]["plan"].info()["n_targets"] == 3 and np.array_equal(np.asarray(m.scene.vertices), sc.vertices)
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        restore(gpu_ctx)


# ---- 3. the temporal protocol -------------------------------------------------------------------------------------------------------
def test_morph_meshes_keeps_the_history_without_a_download(gpu_ctx):
    sc = near_scene()
    nb = N_BLOB[SMALL[1]]
    with Context(gpu_ctx.device) as ctx:
        m = started(ctx, copy.copy(sc))
        m.AttachBlendShapes(0, blob_shapes(sc, nb)[:2])
        m.MorphMeshes({0: np.array([0.4, 0.2], F)}, keep_history=True)
        for _ in range(2):
            m.OnRenderImage()
        m.MorphMeshes({0: np.array([0.8, 0.4], F)}, keep_history=True)
        count = m._tcount.GetPixels()[..., 0]
        on = (m._taov[1][2].GetPixels().view(np.int32)[..., 0] == 0) & (m._taov[1][1].GetPixels()[..., 3] == 3)
        assert on.mean() > 0.02 and (count[on] > 0).mean() >= 0.5, (on.mean(), (count[on] > 0).mean())
        assert ctx.buffer_state(m._vertexBuffer)["downloads"] == 0 and ctx.buffer_state(m._tdeform[0])["downloads"] == 0
        m.MorphMeshes({0: np.array([0.1, 0.9], F)})           # without keep_history: no history on the morphed mesh, as with SkinMeshes
        count = m._tcount.GetPixels()[..., 0]
        on = (m._taov[1][2].GetPixels().view(np.int32)[..., 0] == 0) & (m._taov[1][1].GetPixels()[..., 3] == 3)
        assert on.any() and (count[on] == 0).all() and (count[~on] > 0).mean() >= 0.9
        m.OnDisable()


# ---- 4. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_everything_untouched(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx._h
    gpu_ctx.synchronize()
    P, N, d, w = variant_case("plain", 2, 10, 3, seed=9)        # 15 elements, 2 .. 11 served
    d = np.concatenate([d, M.deltas_array([2, 11], [0, 2], np.ones((2, 3)))])      # both ends of the range and the last target are named
    raw = RawMorph(gpu_ctx, P, N, d, w, 2, 10)
    raw.morph()                                                # (a stale range to keep)
    other12, other4, short12 = ComputeBuffer(gpu_ctx, 16, 12), ComputeBuffer(gpu_ctx, 4, 4), ComputeBuffer(gpu_ctx, 11, 12)
    before = [gpu_ctx.buffer_state(b) for b in raw.all()]
    d0, live0 = gpu_ctx.deform_stats(), live_resources()
    # urt_morph_plan_create
    out = C.c_uint64(77)
    ptr = d.ctypes.data_as(C.c_void_p)

    def create(deltas=ptr, n_deltas=len(d), n_targets=3, first=2, count=10, out_plan=C.byref(out)):
        return lib.urt_morph_plan_create(h, deltas, n_deltas, n_targets, first, count, out_plan)

    assert create(deltas=None) == INVALID_ARGUMENT and create(n_deltas=-1) == INVALID_ARGUMENT
    assert create(count=-1) == INVALID_ARGUMENT and create(first=-1) == INVALID_ARGUMENT and create(first=2 ** 31 - 1) == INVALID_ARGUMENT
    for n_targets in (0, -3, 4097):
        assert create(n_targets=n_targets) == INVALID_ARGUMENT
    assert create(out_plan=None) == INVALID_ARGUMENT
    assert create(first=3) == SCENE and create(count=9) == SCENE and create(n_targets=2) == SCENE
    assert out.value == 0 and live_resources() == live0       # on any error nothing stays allocated
    info = _lib.MorphPlanInfo()
    assert lib.urt_morph_plan_info(h, 0xdead, C.byref(info)) == INVALID_HANDLE and lib.urt_morph_plan_info(h, raw.plan.handle, None) == INVALID_ARGUMENT
    assert lib.urt_morph_plan_release(h, 0xdead) == INVALID_HANDLE and lib.urt_morph_plan_release(h, raw.rest_v.handle) == INVALID_HANDLE
    # urt_morph_vertices
    H = {k: getattr(raw, k).handle for k in ("plan", "rest_v", "rest_n", "weights", "dst_v", "dst_n")}

    def call(flags=0, **over):
        a = dict(H, **over)
        return lib.urt_morph_vertices(h, a["plan"], a["rest_v"], a["rest_n"], a["weights"], a["dst_v"], a["dst_n"], flags)

    assert call(plan=0) == INVALID_HANDLE and call(plan=0xdead) == INVALID_HANDLE and call(plan=H["rest_v"]) == INVALID_HANDLE
    for flags in (2, 3, -1, 1 << 30):
        assert call(flags=flags) == INVALID_ARGUMENT, flags
    assert call(flags=1, rest_n=0, dst_n=0) == INVALID_ARGUMENT                    # URT_MORPH_NORMALIZE without dst_normals
    assert call(rest_n=0) == INVALID_ARGUMENT                                      # dst_normals without rest_normals
    assert call(rest_v=other12.handle) == INVALID_ARGUMENT                         # counts that do not fit
    assert call(dst_v=other12.handle) == INVALID_ARGUMENT and call(dst_n=other12.handle) == INVALID_ARGUMENT
    assert call(weights=other4.handle) == INVALID_ARGUMENT                         # ... the plan has 3 targets
    assert call(rest_v=short12.handle, rest_n=0, dst_v=short12.handle, dst_n=0) == INVALID_ARGUMENT
    assert call(weights=H["rest_v"]) == INVALID_ARGUMENT and call(dst_v=H["weights"]) == INVALID_ARGUMENT       # strides that do not fit
    assert call(rest_n=H["weights"]) == INVALID_ARGUMENT
    assert call(dst_v=H["rest_v"]) == INVALID_ARGUMENT and call(dst_n=H["rest_n"]) == INVALID_ARGUMENT          # a destination equal to an input
    assert call(dst_n=H["rest_v"]) == INVALID_ARGUMENT and call(dst_v=H["rest_n"]) == INVALID_ARGUMENT
    assert call(dst_n=H["dst_v"]) == INVALID_ARGUMENT                              # ... or to the other destination
    for key in ("rest_v", "weights", "dst_v"):
        assert call(**{key: 0}) == INVALID_HANDLE and call(**{key: 0xdead}) == INVALID_HANDLE, key
    assert call(dst_n=0xdead) == INVALID_HANDLE and call(rest_n=0xdead) == INVALID_HANDLE and call(rest_n=0xdead, dst_n=0) == INVALID_HANDLE
    big = ComputeBuffer(gpu_ctx, 11, 12)                                           # 12-byte buffers that end inside the served range
    assert lib.urt_morph_vertices(h, H["plan"], short12.handle, 0, H["weights"], big.handle, 0, 0) == INVALID_ARGUMENT
    assert [gpu_ctx.buffer_state(b) for b in raw.all()] == before and gpu_ctx.deform_stats() == d0
    assert gpu_ctx.buffer_state(short12)["mirror_bytes"] == 0 and gpu_ctx.buffer_state(big)["mirror_bytes"] == 0
    want = M.morph(P, N, d, 2, 10, w)[0]
    got = f32(raw.dst_v)
    assert same(got[2:12], want) and (got[:2] == SENTINEL).all() and (got[12:] == SENTINEL).all()
    raw.release(); other12.Release(); other4.Release(); short12.Release(); big.Release()


# ---- 5. resources -------------------------------------------------------------------------------------------------------------------
def test_resources_return_to_the_baseline(gpu_ctx):
    gpu_ctx.synchronize()
    base = live_resources()
    P, N, d, w = variant_case("plain", 0, 300, 3, seed=2)
    plan = gpu_ctx.morph_plan(d, 3, 0, 300)
    bytes_ = plan.info()["device_bytes"]
    assert bytes_ == 8 * 300 + 28 * len(d) and live_resources()["device_bytes"] >= base["device_bytes"] + bytes_
    plan.Release()
    assert live_resources() == base
    plan.Release()                                            # released already: nothing to do
    with Context(gpu_ctx.device) as ctx:                      # a context destroyed with a live plan, used and unused
        inside = live_resources()
        a, b = ctx.morph_plan(d, 3, 0, 300), ctx.morph_plan(d[:0], 3, 0, 0)
        rv, wv, dv = ComputeBuffer(ctx, 303, 12), ComputeBuffer(ctx, 3, 4), ComputeBuffer(ctx, 303, 12)
        rv.SetData(P); wv.SetData(w)
        a.morph(rv, None, wv, dv, None)
        assert same(f32(dv)[:300], M.morph(P, None, d, 0, 300, w)[0])
        assert live_resources()["device_bytes"] >= inside["device_bytes"] + bytes_ + 2 * 303 * 12 and b.info()["device_bytes"] == 0
    assert live_resources() == base
