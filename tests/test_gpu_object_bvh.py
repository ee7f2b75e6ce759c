"""GPU: the object-level BVH on the device (include/urt.h urt_mesh_leaf_bounds_device, urt_sphere_leaf_bounds_device,
urt_build_object_bvh_device; csrc/object_bvh.hip) against the library's own host functions on the same inputs: integer fields bit for
bit, floats by value (==: -0 equals +0, and no NaN occurs in the contract cases)."""

import numpy as np
import pytest

import skin_ref as S
from unityraytracer_amd import ComputeBuffer, Context, _lib, host_scene, live_resources, scenes

pytestmark = pytest.mark.gpu

F = np.float32
NODE = scenes.BVHNODE_DT
B = _lib.MESH_LEAF_BLOCKS
SENTINEL = F(7.5)
INVALID_ARGUMENT, INVALID_HANDLE, SCENE = 1, 2, 8
HEAP_SIZES = [1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024]


def nodes_of(buf):
    return buf.GetData().reshape(-1).view(NODE).copy()


def sentinel_nodes(n):
    a = np.zeros(n, NODE)
    a["vmin"], a["vmax"], a["index"] = SENTINEL, SENTINEL, 0x5E5E5E5E
    return a


def assert_nodes_equal(got, want, what=""):
    assert got.shape == want.shape, what
    assert np.array_equal(got["index"], want["index"]), what                       # bit for bit
    assert not np.isnan(want["vmin"]).any() and not np.isnan(want["vmax"]).any(), what
    assert (got["vmin"] == want["vmin"]).all() and (got["vmax"] == want["vmax"]).all(), what


def buffer_of(ctx, a, stride):
    a = np.ascontiguousarray(a)
    b = ComputeBuffer(ctx, a.nbytes // stride, stride)
    b.SetData(a)
    return b


def untouched(ctx, buf):
    st = ctx.buffer_state(buf)
    return st["stale_first"] > st["stale_last"] and (buf.GetData().view(F)[:, :6] == SENTINEL).all()


# ---- the synthetic mesh scenes ----------------------------------------------------------------------------------------------------------
def random_matrix(rng):
    """rotation . non-uniform scale . translation, column-major as a MeshObject holds it."""
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    m = np.eye(4)
    m[:3, :3] = q @ np.diag(rng.uniform(0.25, 2.5, 3))
    m[:3, 3] = rng.uniform(-20, 20, 3)
    return m.T.astype(F).reshape(16)


def mesh_scene(slot_counts, seed, shared=(0, 1)):
    """MeshObjects with the given index-slot counts over one vertex pool.  Every mesh draws its indices from a window of the pool of its
    own — the pair `shared` from one common window — with unused vertices between the windows and unused slots between the ranges."""
    rng = np.random.default_rng(seed)
    n = len(slot_counts)
    window, gap = 97, 11
    nv = n * (window + gap)
    v = rng.uniform(-4, 4, (nv, 3)).astype(F)
    special = np.array([0.0, -0.0, 1e-45, -3e-42, 1.1e-38, 9.5e29, -9.9e29, 1e30], F)     # +-0, denormals, values near 1e30
    v[rng.integers(0, nv, 64), rng.integers(0, 3, 64)] = rng.choice(special, 64)
    v[5] = (0.0, -0.0, 1e-45)
    mo = np.zeros(n, scenes.MESHOBJECT_DT)
    idx, at = [], 0
    for m, cnt in enumerate(slot_counts):
        w = shared[0] if (m in shared and len(slot_counts) > max(shared)) else m
        lo = w * (window + gap)
        idx.append(np.full(7, 3, np.int32))                                        # slots no MeshObject names
        at += 7
        mo[m]["localToWorldMatrix"], mo[m]["indices_offset"], mo[m]["indices_count"] = random_matrix(rng), at, cnt
        idx.append(rng.integers(lo, lo + window, cnt).astype(np.int32))
        at += cnt
    idx.append(np.full(5, 2, np.int32))
    return mo, v, np.concatenate(idx)


STRADDLE = [0, 1, 3, 255, 256, 257, 256 * B - 1, 256 * B, 256 * B + 1]
SCENES = {1: [257], 2: [3, 256 * B + 1], 13: STRADDLE + [30, 1000, 6, 12]}


class RawMeshes:
    def __init__(self, ctx, mo, v, idx):
        self.ctx = ctx
        self.mo, self.v, self.idx = buffer_of(ctx, mo, 112), buffer_of(ctx, v, 12), buffer_of(ctx, idx, 4)
        self.leaves = buffer_of(ctx, sentinel_nodes(len(mo)), 28)

    def run(self):
        self.ctx.mesh_leaf_bounds(self.mo, self.v, self.idx, self.leaves)
        st = self.ctx.buffer_state(self.leaves)                                    # enqueued, nothing read yet: the whole range is stale
        assert (st["stale_first"], st["stale_last"], st["mirror_bytes"]) == (0, self.leaves.count - 1, self.leaves.count * 28), st
        return nodes_of(self.leaves)

    def release(self):
        for b in (self.mo, self.v, self.idx, self.leaves):
            b.Release()


@pytest.fixture(scope="module")
def scene13():
    mo, v, idx = mesh_scene(SCENES[13], seed=13)
    return mo, v, idx, host_scene.mesh_leaf_bounds(mo, v, idx)


# ---- mesh leaves ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_meshes", [1, 2, 13])
def test_mesh_leaves_equal_the_host_function(gpu_ctx, n_meshes):
    mo, v, idx = mesh_scene(SCENES[n_meshes], seed=n_meshes)
    want = host_scene.mesh_leaf_bounds(mo, v, idx)
    raw = RawMeshes(gpu_ctx, mo, v, idx)
    got = raw.run()
    assert_nodes_equal(got, want, n_meshes)                                         # every row is written: no sentinel is left
    assert np.array_equal(got["index"], np.arange(n_meshes))
    empty = np.flatnonzero(mo["indices_count"] == 0)
    assert (got["vmin"][empty] == 0).all() and (got["vmax"][empty] == 0).all()
    raw.release()


def test_mesh_leaves_follow_a_skin_on_the_device(gpu_ctx, scene13):
    mo, v, idx, _ = scene13
    n = len(v)
    rng = np.random.default_rng(5)
    rest = rng.uniform(-3, 3, (n, 3)).astype(F)
    normals = rng.normal(size=(n, 3)).astype(F)
    j = rng.integers(0, 3, (n, 4)).astype(np.int32)
    w = rng.uniform(0, 1, (n, 4)).astype(F)
    bones = rng.uniform(-1.5, 1.5, (3, 12)).astype(F)
    skinned, _ = S.skin(rest, normals, j, w, bones)
    raw = RawMeshes(gpu_ctx, mo, v, idx)
    ins = [buffer_of(gpu_ctx, a, s) for a, s in ((rest, 12), (normals, 12), (j, 16), (w, 16), (bones, 48))]
    gpu_ctx.skin_vertices(ins[0], None, ins[2], ins[3], ins[4], 0, n, raw.v, None)
    got = raw.run()
    assert_nodes_equal(got, host_scene.mesh_leaf_bounds(mo, skinned, idx), "skinned")
    assert gpu_ctx.buffer_state(raw.v)["downloads"] == 0                            # the positions never crossed the bus
    raw.release()
    for b in ins:
        b.Release()


def test_slots_with_an_index_outside_the_vertices_are_skipped(gpu_ctx):
    mo, v, idx = mesh_scene([40, 50, 60], seed=77)
    bad = idx.copy()
    first = int(mo[1]["indices_offset"])
    bad[first + 7], bad[first + 31] = -1, len(v)
    mended = idx.copy()
    mended[first + 7] = mended[first + 31] = idx[first]                             # a vertex the mesh names anyway: the same box
    want = host_scene.mesh_leaf_bounds(mo, v, mended)
    raw = RawMeshes(gpu_ctx, mo, v, bad)
    assert_nodes_equal(raw.run(), want, "skipped")
    raw.release()


# ---- sphere leaves ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sphere_leaves_equal_the_host_function(gpu_ctx, n):
    rng = np.random.default_rng(n)
    sp = np.zeros(n, scenes.SPHERE_DT)
    sp["position"] = rng.uniform(-50, 50, (n, 3)).astype(F)
    sp["radius"] = rng.uniform(0.1, 5, n).astype(F)
    sp["radius"][0] = 0.0
    sp["radius"][n // 2] = -2.5 if n > 1 else 0.0
    if n > 2:
        sp["radius"][n - 1], sp["position"][n - 1] = -0.0, (0.0, -0.0, 1e-40)
    spheres, leaves = buffer_of(gpu_ctx, sp, 56), buffer_of(gpu_ctx, sentinel_nodes(n), 28)
    gpu_ctx.sphere_leaf_bounds(spheres, leaves)
    assert_nodes_equal(nodes_of(leaves), host_scene.sphere_leaf_bounds(sp), n)
    spheres.Release(); leaves.Release()


# ---- the heap ---------------------------------------------------------------------------------------------------------------------------
def heap_inputs(n):
    rng = np.random.default_rng(1000 + n)
    out = {}
    a = np.zeros(n, NODE)
    a["vmin"] = rng.uniform(-10, 10, (n, 3)).astype(F)
    a["vmax"] = a["vmin"] + rng.uniform(0, 3, (n, 3)).astype(F)
    a["index"] = np.arange(n)
    out["random"] = a
    b = a.copy()
    b["vmin"], b["vmax"] = a["vmin"][0], a["vmax"][0]
    out["identical"] = b                                                           # every tie falls to the leaf number
    g = a.copy()
    c = rng.integers(0, 4, (n, 3)).astype(F)                                       # exact ties on the chosen axis, equal extents on two or three axes
    g["vmin"], g["vmax"] = c - F(0.5), c + F(0.5)
    out["grid"] = g
    sp = np.zeros(n, scenes.SPHERE_DT)
    sp["position"], sp["radius"] = rng.uniform(-9, 9, (n, 3)).astype(F), rng.uniform(0.1, 2, n).astype(F)
    out["inverted"] = host_scene.sphere_leaf_bounds(sp, literal=True)
    p = a.copy()
    p["index"] = rng.permutation(n) * 3 + 5                                         # the leaves' own index fields, copied verbatim
    out["permuted"] = p
    return out


def device_heap(ctx, leaves_in):
    n = len(leaves_in)
    length = host_scene.build_object_bvh(leaves_in).shape[0]
    leaves, heap = buffer_of(ctx, leaves_in, 28), buffer_of(ctx, sentinel_nodes(length), 28)
    ctx.build_object_bvh(leaves, heap)
    st = ctx.buffer_state(heap)
    assert (st["stale_first"], st["stale_last"]) == (0, length - 1), n
    got = nodes_of(heap)
    leaves.Release(); heap.Release()
    return got


@pytest.mark.parametrize("n", HEAP_SIZES)
def test_heap_equals_the_host_builder(gpu_ctx, n):
    for name, leaves in heap_inputs(n).items():
        want = host_scene.build_object_bvh(leaves)
        assert_nodes_equal(device_heap(gpu_ctx, leaves), want, (name, n))          # filler nodes included: no sentinel is left


def test_chain_equals_the_host_chain(gpu_ctx, scene13):
    mo, v, idx, host_leaves = scene13
    want = host_scene.build_object_bvh(host_leaves)
    raw = RawMeshes(gpu_ctx, mo, v, idx)
    heap = buffer_of(gpu_ctx, sentinel_nodes(len(want)), 28)
    gpu_ctx.mesh_leaf_bounds(raw.mo, raw.v, raw.idx, raw.leaves)
    gpu_ctx.build_object_bvh(raw.leaves, heap)                                      # reads the leaves where the first call wrote them
    assert_nodes_equal(nodes_of(heap), want, "chain")
    assert gpu_ctx.buffer_state(raw.leaves)["downloads"] == 0
    raw.release(); heap.Release()


def test_non_finite_leaves_give_a_well_formed_heap(gpu_ctx):
    n = 65
    leaves = heap_inputs(n)["random"]
    rng = np.random.default_rng(9)
    for value in (np.nan, np.inf, -np.inf):
        rows = rng.integers(0, n, 9)
        leaves["vmin"][rows, rng.integers(0, 3, 9)] = value
        leaves["vmax"][rng.integers(0, n, 9), rng.integers(0, 3, 9)] = value
    got = device_heap(gpu_ctx, leaves)                                             # outside the contract: no error, and
    assert len(got) == 255
    named = got["index"][got["index"] >= 0]
    assert np.array_equal(np.sort(named), np.arange(n))                            # every leaf exactly once,
    assert (got["index"][got["index"] < 0] == -1).all()                            # interior and filler nodes carry -1
    topo = host_scene.build_object_bvh(heap_inputs(n)["random"])                    # the topology depends on n alone
    assert np.array_equal(got["index"] >= 0, topo["index"] >= 0)


# ---- errors: nothing is enqueued or marked ----------------------------------------------------------------------------------------------
def test_errors_leave_the_destinations_untouched(gpu_ctx):
    ctx, lib, h = gpu_ctx, gpu_ctx.lib, gpu_ctx._h
    mo, v, idx = mesh_scene([30, 40, 50], seed=3)
    raw = RawMeshes(ctx, mo, v, idx)
    sp = np.zeros(3, scenes.SPHERE_DT)
    spheres, sleaves = buffer_of(ctx, sp, 56), buffer_of(ctx, sentinel_nodes(3), 28)
    heap3 = buffer_of(ctx, sentinel_nodes(7), 28)
    wrong = {s: buffer_of(ctx, np.zeros((3, s // 4), F), s) for s in (112, 12, 4, 28, 56)}
    M, V, I, L = raw.mo.handle, raw.v.handle, raw.idx.handle, raw.leaves.handle
    dests = (raw.leaves, sleaves, heap3)

    def check(rc, want):
        assert rc == want
        assert all(untouched(ctx, d) for d in dests)

    # every wrong stride
    check(lib.urt_mesh_leaf_bounds_device(h, wrong[12].handle, V, I, L), INVALID_ARGUMENT)
    check(lib.urt_mesh_leaf_bounds_device(h, M, wrong[4].handle, I, L), INVALID_ARGUMENT)
    check(lib.urt_mesh_leaf_bounds_device(h, M, V, wrong[12].handle, L), INVALID_ARGUMENT)
    check(lib.urt_mesh_leaf_bounds_device(h, M, V, I, wrong[12].handle), INVALID_ARGUMENT)
    check(lib.urt_sphere_leaf_bounds_device(h, wrong[112].handle, sleaves.handle), INVALID_ARGUMENT)
    check(lib.urt_sphere_leaf_bounds_device(h, spheres.handle, wrong[12].handle), INVALID_ARGUMENT)
    check(lib.urt_build_object_bvh_device(h, wrong[12].handle, heap3.handle), INVALID_ARGUMENT)
    check(lib.urt_build_object_bvh_device(h, sleaves.handle, wrong[4].handle), INVALID_ARGUMENT)
    # every wrong count
    four = buffer_of(ctx, sentinel_nodes(4), 28)
    check(lib.urt_mesh_leaf_bounds_device(h, M, V, I, four.handle), INVALID_ARGUMENT)
    check(lib.urt_sphere_leaf_bounds_device(h, spheres.handle, four.handle), INVALID_ARGUMENT)
    check(lib.urt_build_object_bvh_device(h, sleaves.handle, four.handle), INVALID_ARGUMENT)      # 3 leaves: 7 nodes
    assert untouched(ctx, four)
    # more leaves than the device builder takes
    many = buffer_of(ctx, sentinel_nodes(_lib.OBJECT_BVH_DEVICE_MAX + 1), 28)
    big = buffer_of(ctx, sentinel_nodes(4095), 28)
    check(lib.urt_build_object_bvh_device(h, many.handle, big.handle), INVALID_ARGUMENT)
    assert b"urt_host_build_object_bvh" in lib.urt_last_error(h) and untouched(ctx, big)
    # a destination equal to an input
    one = buffer_of(ctx, sentinel_nodes(1), 28)
    check(lib.urt_build_object_bvh_device(h, one.handle, one.handle), INVALID_ARGUMENT)
    check(lib.urt_mesh_leaf_bounds_device(h, M, V, I, M), INVALID_ARGUMENT)
    check(lib.urt_sphere_leaf_bounds_device(h, spheres.handle, spheres.handle), INVALID_ARGUMENT)
    assert untouched(ctx, one)
    # a handle that is 0, and an unknown handle
    for bad in (0, 0xdead):
        for k in range(4):
            args = [M, V, I, L]
            args[k] = bad
            check(lib.urt_mesh_leaf_bounds_device(h, *args), INVALID_HANDLE)
        check(lib.urt_sphere_leaf_bounds_device(h, bad, sleaves.handle), INVALID_HANDLE)
        check(lib.urt_sphere_leaf_bounds_device(h, spheres.handle, bad), INVALID_HANDLE)
        check(lib.urt_build_object_bvh_device(h, bad, heap3.handle), INVALID_HANDLE)
        check(lib.urt_build_object_bvh_device(h, sleaves.handle, bad), INVALID_HANDLE)
    # a MeshObject range beyond indices
    for field, value in (("indices_offset", -1), ("indices_count", -1), ("indices_count", len(idx))):
        broken = mo.copy()
        broken[2][field] = value
        raw.mo.SetData(broken)
        check(lib.urt_mesh_leaf_bounds_device(h, M, V, I, L), SCENE)
    raw.mo.SetData(mo)
    assert_nodes_equal(raw.run(), host_scene.mesh_leaf_bounds(mo, v, idx), "after the errors")
    for b in (spheres, sleaves, heap3, four, many, big, one) + tuple(wrong.values()):
        b.Release()
    raw.release()


# ---- resources --------------------------------------------------------------------------------------------------------------------------
def test_resources_return_to_the_baseline(gpu_ctx):
    gpu_ctx.synchronize()
    base = live_resources()
    mo, v, idx = mesh_scene([300, 5], seed=1)
    with Context(gpu_ctx.device) as ctx:
        raw = RawMeshes(ctx, mo, v, idx)
        heap = buffer_of(ctx, sentinel_nodes(3), 28)
        raw.run()
        ctx.build_object_bvh(raw.leaves, heap)
        ctx.synchronize()
        assert live_resources()["device_bytes"] >= base["device_bytes"] + 2 * B * 32      # the mirrors and the partials' scratch
        raw.release(); heap.Release()
    assert live_resources() == base
