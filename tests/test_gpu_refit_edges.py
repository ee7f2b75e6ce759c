"""GPU: the refit of moved MeshObjects (csrc/refit.hip) against its exact restatement (tests/refit_ref.py), on trees of every builder and
leaf size, through the poses of tests/test_refit_ref.py (many or all MeshObjects at once, mirrors, scale 0, a flattened axis, 1e5 away
and back, scales of 1e3 and 1e-3, an arbitrary rotation with non-uniform scale, ten refits that end at the start).  After every step:
(a) the read-back nodes equal the restatement bit for bit, (b) every box holds its triangles with half a pad of margin (float64),
(c) the frame equals the oracle's literal walk and a from-scratch preparation, (d) ray queries aimed at moved vertices and edges and
grazing refitted leaf boxes equal the oracle (literal walk, and culled walk on the read-back tree), any-hit included, and (e) the step was
a refit in place.  Then a stale object-level heap: a MeshObject moved out of its heap leaf box with only _MeshObjects re-uploaded must lose
its object-level cull and get it back when it returns (csrc/cullflags.hip), with traversal counters equal to the oracle's."""
import copy

import numpy as np
import pytest

import qnodes_ref as Q
import refit_ref as R
from oracle import pyoracle
from test_gpu_ray_query import assert_matches_oracle, oracle_trace
from test_gpu_refit import bits_equal, fresh_frame, reupload
from test_refit_ref import SCENES, apply, local, pose_steps, world
from unityraytracer_amd import Context, RayTraceMaster

pytestmark = pytest.mark.gpu

F = np.float32
RESTORE = {"blas_builder": -1, "blas_leaf_max": 2, "qnodes": 0, "count_stats": 0, "kernel_mode": 3, "refit": 1}


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


def leaf_sizes(sc, nodes, tri):
    """Triangles per leaf child of the nodes, a leaf whose triangles all have one box (so one centroid: the host builder keeps such a
    group, like a quad's two halves, in one leaf whatever blas_leaf_max says) counted as 1."""
    kids = np.asarray(nodes, F)[:, 12:14].view(np.int32).reshape(-1)
    first, cnt = R.leaf_range(kids[kids < 0])
    w = R.records(sc, tri)["w"]
    lo, hi = w.min(axis=1), w.max(axis=1)
    same = np.array([(lo[f:f + c] == lo[f]).all() and (hi[f:f + c] == hi[f]).all() for f, c in zip(first, cnt)], bool)
    return np.where(same, 1, cnt)


def probe_rays(rng, sc, nodes, tri, root, moved, n=48):
    """Rays at the vertices and edge midpoints of moved triangles (as the triangle test reconstructs them), and rays that start one ulp
    outside a face of a refitted leaf box and run along it (components 0, -0 or 1e-7 across the face, sometimes a second zero)."""
    rec = R.records(sc, tri)
    pts = R.reconstructed(rec).astype(np.float64)
    mv = np.nonzero((rec["mesh"] >= 0) & moved[np.maximum(rec["mesh"], 0)])[0]
    O, D = [], []
    for i, t in enumerate(rng.choice(mv, n) if len(mv) else []):
        v = pts[t]
        target = v[i % 3] if i % 2 == 0 else 0.5 * (v[i % 3] + v[(i + 1) % 3])
        o = target + rng.normal(size=3) * 3.0 * max(1.0, 1e-3 * np.abs(v).max())
        O.append(o), D.append(target - o)
    kids, node_mesh, _ = R.topology(nodes, root)
    boxes = [(a, k) for a in np.nonzero((node_mesh >= 0) & moved[np.maximum(node_mesh, 0)])[0] for k in range(2) if kids[a, k] < 0]
    for j in (rng.choice(len(boxes), n) if boxes else []):
        a, k = boxes[j]
        lo, hi = nodes[a, 6 * k: 6 * k + 3], nodes[a, 6 * k + 3: 6 * k + 6]
        ax = int(rng.integers(3))
        o = (lo + rng.random(3).astype(F) * (hi - lo)).astype(F)
        d = rng.normal(size=3).astype(F)
        below = rng.random() < 0.5
        o[ax] = np.nextafter(lo[ax], -np.inf) if below else np.nextafter(hi[ax], np.inf)
        d[ax] = [F(0.0), F(-0.0), F(1e-7) if below else F(-1e-7)][int(rng.integers(3))]
        if rng.random() < 0.3:
            d[(ax + 1) % 3] = F(-0.0) if rng.random() < 0.5 else F(0.0)
        O.append(o), D.append(d)
    return np.array(O, F).reshape(-1, 3), np.array(D, F).reshape(-1, 3)


def check_step(ctx, other, m, builder, cur, nxt, nodes, tri, root, rng, what, qnodes=0):
    """One pose step: re-upload as RebuildTrees does, render, and check (a) to (e).  -> the read-back nodes."""
    moved = R.moved_meshes(cur, nxt)
    r0, p0 = ctx.refit_stats()
    built0 = ctx.blas_cache_stats()[1]
    reupload(m, nxt)
    m.OnRenderImage()
    got = m._target.GetPixels()
    new, tri2, root2, _ = ctx.read_scene_blas(len(nxt.mesh_objects))
    # (e) a refit in place, of exactly the moved MeshObjects
    r1, p1 = ctx.refit_stats()
    assert (r1 - r0, p1 - p0) == (int(moved.sum()), 1), (what, r1 - r0, p1 - p0, int(moved.sum()))
    assert builder != 0 or ctx.blas_cache_stats()[1] == built0, what
    assert np.array_equal(tri2, tri) and np.array_equal(root2, root), what
    # (a) the nodes == the restatement, bit for bit
    want, pad = R.refit(nxt, nodes, tri, root, moved)
    diff = (new.view(np.uint32) != want.view(np.uint32)).any(axis=1)
    if diff.any():
        _, node_mesh, depth = R.topology(nodes, root)
        bad = np.nonzero(diff)[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(new)} nodes differ from the restatement (MeshObjects {sorted(set(node_mesh[bad].tolist()))[:8]}, "
                             f"depths {sorted(set(depth[bad].tolist()))[:8]}); first {bad[0]}: gpu {new[bad[0], :12].tolist()} want {want[bad[0], :12].tolist()}")
    # (b) containment with margin, tight on the refitted MeshObjects
    res = R.check_boxes(nxt, new, tri, root, pad, tight=moved)
    assert R.failures(res) == 0 and res["min_margin"] >= 0.5, (what, res)
    # (c) frames: the oracle's literal walk, a from-scratch preparation
    o = pyoracle.Oracle(nxt)
    assert bits_equal(got, o.render(mode=0, threads=8)), f"{what}: frame differs from the oracle's literal walk"
    if qnodes:
        frame, words, _ = ctx.read_scene_qnodes()
        rf, rw = Q.quantized_nodes(new, root)
        assert bits_equal(frame, rf) and np.array_equal(words, rw), f"{what}: quantized nodes differ from their restatement"
        other.set_option("qnodes", qnodes)
    assert bits_equal(got, fresh_frame(other, nxt, builder)), f"{what}: frame differs from a from-scratch preparation"
    # (d) ray queries: literal walk and culled walk on the read-back tree, closest and any hit
    O, D = probe_rays(rng, nxt, new, tri, root, moved)
    if len(O):
        hits = ctx.ray_query(O, D)
        ref = oracle_trace(o, O, D, mode=0)
        assert_matches_oracle(hits, ref, f"{what}: rays vs the literal walk")
        o1 = pyoracle.Oracle(nxt)
        o1.set_blas(new, tri, root)
        assert_matches_oracle(hits, oracle_trace(o1, O, D, mode=1), f"{what}: rays vs the culled walk on the read-back tree")
        dist = ref[:, 0]
        assert np.array_equal(ctx.ray_query(O, D, any_hit=True), (dist < np.inf).astype(np.int32)), what
        t = np.where(np.isfinite(dist), dist * rng.uniform(0.5, 1.5, len(dist)), rng.uniform(0, 50, len(dist))).astype(F)
        t[::5] = dist[::5]
        assert np.array_equal(ctx.ray_query(O, D, t_max=t, any_hit=True), (dist < t).astype(np.int32)), what
    return new


def run_poses(ctx, other, name, builder, leaf, qnodes=0):
    sc = SCENES[name]()
    try:
        ctx.set_option("kernel_mode", 3)
        ctx.set_option("blas_leaf_max", leaf)          # (process-wide: the second context's preparations follow)
        ctx.set_option("blas_builder", builder)
        ctx.set_option("qnodes", qnodes)
        m = RayTraceMaster(ctx, sc)
        m.OnRenderImage()
        nodes, tri, root, _ = ctx.read_scene_blas(len(sc.mesh_objects))
        sizes = leaf_sizes(sc, nodes, tri)
        assert sizes.max() <= leaf and (name == "deep_chain" or leaf == 1 or sizes.max() > 1), (name, builder, leaf, sizes.max())
        rng = np.random.default_rng(1000 * builder + leaf)
        cur = sc
        for step, edits in pose_steps(sc):
            nxt = apply(cur, edits)
            nodes = check_step(ctx, other, m, builder, cur, nxt, nodes, tri, root, rng, f"{name} builder {builder} leaf {leaf} qnodes {qnodes}: {step}", qnodes)
            cur = nxt
        assert ctx.counters()["watchdog_trips"] == 0
        m.OnDisable()
        ctx.synchronize()
    finally:
        other.set_option("qnodes", 0)
        restore(ctx)


@pytest.mark.parametrize("builder", [0, 1, 2, 3])
@pytest.mark.parametrize("name", list(SCENES))
def test_poses_on_every_builder(gpu_ctx, other_ctx, name, builder):
    run_poses(gpu_ctx, other_ctx, name, builder, 2)


@pytest.mark.parametrize("leaf", [1, 4, 8])
@pytest.mark.parametrize("builder", [0, 3])
@pytest.mark.parametrize("name", ["mixed", "c5_small"])
def test_poses_on_other_leaf_sizes(gpu_ctx, other_ctx, name, builder, leaf):
    run_poses(gpu_ctx, other_ctx, name, builder, leaf)


def test_poses_with_quantized_nodes(gpu_ctx, other_ctx):
    """qnodes = 1: after every refit the quantized copy is re-derived (rederive_nodes) and equals its restatement of the refitted nodes."""
    run_poses(gpu_ctx, other_ctx, "mixed", 0, 2, qnodes=1)


# ---- a stale object-level heap through the refit path --------------------------------------------------------------------------------
def counted_frame(ctx, m):
    m._frame = 0; m._currentSample = 0
    ctx.reset_counters()
    m.OnRenderImage()
    return m._target.GetPixels(), ctx.counters()


def stale_check(ctx, m, sc, what):
    """The frame and its traversal counters == the oracle of the same (stale) scene: culled walk on the read-back tree with the oracle's
    own cull flags, and the pixels of the literal walk.  -> the oracle's cull flags."""
    got, gc = counted_frame(ctx, m)
    nodes, tri, root, _ = ctx.read_scene_blas(len(sc.mesh_objects))
    o = pyoracle.Oracle(sc)
    o.set_blas(nodes, tri, root)
    ref, oc = o.render(mode=1, threads=8, counters=True)
    assert bits_equal(got, ref), f"{what}: frame differs from the oracle's culled walk"
    assert bits_equal(got, o.render(mode=0, threads=8)), f"{what}: frame differs from the oracle's literal walk"
    for k in ("tlas_nodes", "blas_nodes", "tri_tests", "hit_tri", "hit_sky"):
        assert gc[k] == oc[k], (what, k, gc[k], oc[k])
    assert gc["watchdog_trips"] == 0
    return o.cull_flags()


@pytest.mark.parametrize("name,k", [("mixed", 1), ("many_meshes", 40)])
def test_stale_heap_through_the_refit(gpu_ctx, name, k):
    """mixed: a 7-node mesh heap (the masked walk table, k_cull_mask); many_meshes: 255 nodes.  MeshObject k leaves its heap leaf box
    with _MeshBVH left as it was: its cull word must be cleared; back inside, it must be set again (flags are re-derived on every update)."""
    sc = SCENES[name]()
    assert (len(sc.mesh_bvh) <= 31) == (name == "mixed")
    try:
        gpu_ctx.set_option("kernel_mode", 3)
        gpu_ctx.set_option("count_stats", 1)
        m = RayTraceMaster(gpu_ctx, sc)
        flags0 = stale_check(gpu_ctx, m, sc, f"{name} before")
        assert flags0[k] == 1, flags0
        base = np.asarray(sc.mesh_objects["localToWorldMatrix"], F).reshape(-1, 16)
        poses = [("out", world(base[k], (1.5, 0.4, -1.0), 25.0)),            # out of its heap leaf box
                 ("mirrored out", local(base[k], (-1.3, 1, 1))),
                 ("in", local(base[k], 0.8)),                                  # inside the old box again (shrunk about its own origin)
                 ("home", base[k])]
        for step, mat in poses:
            cur = copy.copy(sc)
            mo = sc.mesh_objects.copy()
            mo[k]["localToWorldMatrix"] = mat
            cur.mesh_objects = mo                                              # mesh_bvh: the heap of the start, stale
            r0, p0 = gpu_ctx.refit_stats()
            m._meshObjectBuffer.SetData(mo)
            flags = stale_check(gpu_ctx, m, cur, f"{name} {step}")
            r1, p1 = gpu_ctx.refit_stats()
            assert (r1 - r0, p1 - p0) == (1, 1), (name, step)
            expect = 0 if "out" in step else 1
            assert flags[k] == expect and (np.delete(flags, k) == np.delete(flags0, k)).all(), (name, step, flags)
        m.OnDisable()
        gpu_ctx.synchronize()
    finally:
        restore(gpu_ctx)
