"""GPU: the tile entry table of option "tile_entry" (csrc/tile_entry.h, csrc/tile_entry.hip, front_device.h tile_entry_start).
1. Frames traced with the table equal the frames traced without it and the oracle's, bit for bit — the traced frame and the accumulated
   image, no watchdog trip: a reduced C3, frames of 1 x 1, 65 x 3 and 7 x 130, the close-up, the camera inside the mesh's box, the mesh behind
   the camera, a tessellated floor near / far (moved by 1e4) / along the axes (direction components 0), the deep chain (the stack bound),
   three rays per pixel, both ranks of a two-rank strip split, a 64-frame launch.
2. A launch that may not use the table runs without it, urt_launch_info says so, and the images equal those of option 0: pixel offsets
   outside [0, 1], two cameras inside one batch; a camera change, a vertex deformation with refit and a toggle of "blas_cones" between
   launches rebuild the table; spheres switch it off.
3. With count_stats the counters equal the oracle's (the counting instantiation walks from the root).
4. Conservativeness: for every tile of a 96 x 64 frame, rays through the four extreme sample positions and 32 random ones are sent through
   the batched closest-hit query; no hit triangle lies outside the subtrees the tile lists, no ray of an empty tile hits the mesh."""

import numpy as np
import pytest

from oracle import pyoracle
from unityraytracer_amd import RayTraceMaster, scenes

pytestmark = pytest.mark.gpu

RESTORE = {"tile_entry": -1, "count_stats": 0, "kernel_mode": 3, "blas_cones": -1, "frames_per_launch": 0, "refit": 1}
DONE = -2 ** 31


def restore(ctx):
    for k, v in RESTORE.items():
        ctx.set_option(k, v)


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def diff(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).any(axis=2).sum())


def floor_scene(kind, width, height):
    """One tessellated floor (512 triangles) seen from a low camera: near the world's origin, moved with its camera by 1e4 in x and z, or
    from a level, unrotated camera on an image of odd width and height (direction components of exactly 0)."""
    off = np.array([1e4, 0.0, 1e4]) if kind == "far" else np.zeros(3)
    b = scenes.MeshSceneBuilder()
    b.add(*scenes.grid_quad(off + (-1, 0.5, -1), (2, 0, 0), (0, 0, 2), 16, (0, -1, 0)), scenes.trs(),
          scenes._params((0.7, 0.7, 0.7), (0.1, 0.1, 0.1), (0, 0, 0), 0.4))
    mo, vv, ii, nn, bvh = b.finish()
    sc = scenes.Scene(f"floor-{kind}", width, height, 3, 1, mesh_objects=mo, vertices=vv, indices=ii, normals=nn, mesh_bvh=bvh, sky=scenes.make_sky(64, 32))
    cam = dict(position=(0.0, 1.0, -4.0), fov_deg=60.0) if kind == "axis" else \
        dict(position=tuple(np.add((0.3, 0.9, -2.6), off)), pitch_deg=14.0, yaw_deg=8.0, fov_deg=70.0)
    return sc.resized(width, height, **cam)


def c3(width=96, height=64, **cam):
    sc = scenes.config3(width, height, slices=40, stacks=31, sky=scenes.make_sky(64, 32))
    return sc.resized(width, height, **cam) if cam else sc


def case(name):
    """(scene, frames, master arguments)"""
    if name == "C3":
        return c3(), 4, {}
    if name in ("1x1", "65x3", "7x130"):
        w, h = (int(v) for v in name.split("x"))
        return c3(w, h), 2, {}
    if name == "close-up":
        return c3(position=(0.0, 2.4, -7.3)), 2, {}
    if name == "inside":
        return c3(position=(0.3, 2.0, -4.2), yaw_deg=25.0), 2, {}
    if name == "behind":
        return c3(position=(0.0, 1.5, -1.0)), 2, {}          # the camera looks along +z, the mesh stands at z = -4
    if name in ("near", "far", "axis"):
        return floor_scene(name, 97, 61), 2, {}
    if name == "deep-chain":
        return scenes.deep_chain_scene(96, 64), 2, {}
    if name == "three-rays":
        sc = c3(64, 40)
        sc.num_rays, sc.num_bounces = 3, 4
        return sc, 2, {}
    if name in ("rank0", "rank1"):
        return c3(96, 72), 3, {"rank": int(name[-1]), "world_size": 2}
    if name == "64-frames":
        return c3(48, 32), 64, {}
    raise ValueError(name)


def trace(ctx, sc, frames, tile_entry, **master):
    ctx.set_option("tile_entry", tile_entry)
    m = RayTraceMaster(ctx, sc, **master)
    for _ in range(frames):
        m.OnRenderImage()
    t, c = m._target.GetPixels(), m._converged.GetPixels()
    info = ctx.launch_info()
    tree = ctx.read_scene_blas(len(sc.mesh_objects))[:3]
    m.OnDisable()
    return t, c, info, tree


def oracle_frames(sc, tree, frames, rows=None):
    o = pyoracle.Oracle(sc)
    o.set_blas(*tree)
    acc, img = np.zeros((sc.height, sc.width, 4), np.float32), None
    for f in range(frames):
        ox, oy, sd = scenes.frame_uniforms(f)
        o.set_frame((ox, oy), sd)
        img = o.render(mode=1, threads=8)
        if rows is not None:
            img[~rows] = 0
        acc = pyoracle.accumulate(img, acc, f)
    return img, acc


CASES = ["C3", "1x1", "65x3", "7x130", "close-up", "inside", "behind", "near", "far", "axis", "deep-chain", "three-rays", "rank0", "rank1", "64-frames"]


@pytest.mark.parametrize("name", CASES)
def test_frames_bit_exact(gpu_ctx, name):
    sc, frames, master = case(name)
    sc.num_bounces = min(sc.num_bounces, 8)
    try:
        t0, c0, i0, tree = trace(gpu_ctx, sc, frames, 0, **master)
        t1, c1, i1, _ = trace(gpu_ctx, sc, frames, 1, **master)
        assert i0["tile_entry"] == 0 and i0["tile_entry_k"] == 0, i0
        assert i1["tile_entry"] == 1 and i1["tile_entry_k"] == 8 and i1["blas_stack"] >= 8, i1
        for i in (i0, i1):
            assert i["kernel_mode"] == 3 and i["front_mode"] == 0 and i["kernel"].startswith("k_sched<false, ") and i["kernel"].endswith(", false>"), i     # not counting, no quantized nodes
        if name == "64-frames":
            assert i1["n_frames"] == 64, i1
        rows = None
        if master:
            rows = np.zeros(sc.height, bool)
            for g in range(master["rank"], (sc.height + 7) // 8, master["world_size"]):
                rows[g * 8:(g + 1) * 8] = True
        img, acc = oracle_frames(sc, tree, frames, rows)
        if rows is not None:                                   # (the blend runs over the whole image; outside the rank's strips it blends zeros)
            acc[~rows], c0[~rows], c1[~rows] = 0, 0, 0
        assert same(t1, t0) and same(c1, c0), f"{name}: tile_entry 1 differs from 0 in {diff(t1, t0)} / {diff(c1, c0)} pixels"
        assert same(t1, img) and same(c1, acc), f"{name}: tile_entry 1 differs from the oracle in {diff(t1, img)} / {diff(c1, acc)} pixels"
        assert gpu_ctx.counters()["watchdog_trips"] == 0
    finally:
        restore(gpu_ctx)


def test_auto_is_on_and_the_table_is_cached_across_launches(gpu_ctx):
    sc = c3()
    try:
        # auto builds a table once the camera has stood still: not for a first launch of one frame, for the next launch with that camera
        gpu_ctx.set_option("frames_per_launch", 1)
        m = RayTraceMaster(gpu_ctx, c3(position=(0.5, 1.1, -9.5)))
        first = []
        for _ in range(2):
            m.OnRenderImage()
            m._target.GetPixels()
            first.append(gpu_ctx.launch_info()["tile_entry"])
        m.OnDisable()
        assert first == [0, 1], first
        gpu_ctx.set_option("frames_per_launch", 2)
        m = RayTraceMaster(gpu_ctx, sc)
        for _ in range(6):                                    # three launches, one camera
            m.OnRenderImage()
        m._target.GetPixels()
        info = gpu_ctx.launch_info()
        table, builds = gpu_ctx.read_tile_entry()
        for _ in range(2):
            m.OnRenderImage()
        m._target.GetPixels()
        _, builds2 = gpu_ctx.read_tile_entry()
        m.OnDisable()
        assert info["tile_entry"] == 1 and info["n_frames"] == 2, info
        assert table.shape == (8, 12, 8) and builds2 == builds, (table.shape, builds, builds2)
        assert (table[:, :, 0] != DONE).any() and (table[:, :, 0] == DONE).any()      # the mesh fills part of the frame
    finally:
        restore(gpu_ctx)


def two_frames(ctx, sc, tile_entry, between):
    """Two frames of RM's protocol with `between(master)` run after the first; returns both launches' infos, the images and the builds."""
    ctx.set_option("tile_entry", tile_entry)
    m = RayTraceMaster(ctx, sc)
    m.OnRenderImage()
    t_a = m._target.GetPixels()
    info_a = ctx.launch_info()
    builds_a = ctx.read_tile_entry()[1]
    between(m)
    m.OnRenderImage()
    t_b, c_b = m._target.GetPixels(), m._converged.GetPixels()
    info_b = ctx.launch_info()
    builds_b = ctx.read_tile_entry()[1]
    m.OnDisable()
    return (info_a, info_b), (t_a, t_b, c_b), builds_b - builds_a


@pytest.mark.parametrize("offset", [(1.5, 0.5), (0.5, -0.25)])
def test_pixel_offsets_outside_the_unit_square_switch_it_off(gpu_ctx, offset):
    sc = c3()
    sc.pixel_offset = offset                                   # frame 0 of a master takes the scene's own offset
    try:
        t0, c0, i0, _ = trace(gpu_ctx, sc, 1, 0)
        t1, c1, i1, _ = trace(gpu_ctx, sc, 1, 1)
        assert i0["tile_entry"] == 0 and i1["tile_entry"] == 0, (i0, i1)
        assert same(t1, t0) and same(c1, c0)
        sc.pixel_offset = (1.0, 0.0)                           # the closed ends of the range are in
        t2, _, i2, _ = trace(gpu_ctx, sc, 1, 1)
        t3, _, _, _ = trace(gpu_ctx, sc, 1, 0)
        assert i2["tile_entry"] == 1 and same(t2, t3), i2
    finally:
        restore(gpu_ctx)


def test_two_cameras_inside_one_batch_switch_it_off(gpu_ctx):
    other = scenes.camera_matrices(96, 64, position=(0.4, 1.2, -9.0))

    def run(tile_entry):
        gpu_ctx.set_option("tile_entry", tile_entry)
        gpu_ctx.set_option("frames_per_launch", 4)
        m = RayTraceMaster(gpu_ctx, c3())
        m.OnRenderImage(); m.OnRenderImage()
        m.scene.camera_to_world, m.scene.camera_inverse_projection = other      # (no restart: the next frames join the same batch)
        m.OnRenderImage(); m.OnRenderImage()
        t, c = m._target.GetPixels(), m._converged.GetPixels()
        info = gpu_ctx.launch_info()
        m.OnDisable()
        return t, c, info

    try:
        t0, c0, i0 = run(0)
        t1, c1, i1 = run(1)
        assert i0["n_frames"] == 4 and i1["n_frames"] == 4 and i0["tile_entry"] == 0 and i1["tile_entry"] == 0, (i0, i1)
        assert same(t1, t0) and same(c1, c0)
    finally:
        restore(gpu_ctx)


def turn_camera(m):
    m.MoveCamera(scenes.camera_matrices(96, 64, position=(1.5, 1.8, -9.0), yaw_deg=-8.0)[0])


def swell(m):
    lo, hi = m.vertex_span(0)
    v = np.array(m.scene.vertices[lo:hi + 1], np.float32)
    c = v.mean(axis=0)
    m.DeformMeshes({0: c + (v - c) * np.float32(1.25)})


@pytest.mark.parametrize("what", ["camera", "deform"])
def test_a_camera_change_and_a_refit_between_launches_rebuild_the_table(gpu_ctx, what):
    between = turn_camera if what == "camera" else swell
    try:
        deformed = gpu_ctx.deform_stats()["deformed"]
        i0, img0, _ = two_frames(gpu_ctx, c3(), 0, between)
        i1, img1, rebuilt = two_frames(gpu_ctx, c3(), 1, between)
        assert [i["tile_entry"] for i in i0] == [0, 0] and [i["tile_entry"] for i in i1] == [1, 1], (i0, i1)
        assert rebuilt == 1, rebuilt
        if what == "deform":
            assert gpu_ctx.deform_stats()["deformed"] == deformed + 2      # refitted in place, in both runs
        for a, b in zip(img1, img0):
            assert same(a, b), f"{what}: {diff(a, b)} pixels differ from tile_entry 0"
        assert not same(img1[0], img1[1])                      # (the second frame really shows something else)
        assert gpu_ctx.counters()["watchdog_trips"] == 0
    finally:
        restore(gpu_ctx)


def test_a_toggle_of_the_cones_rebuilds_the_table(gpu_ctx):
    def toggle(m):
        gpu_ctx.set_option("blas_cones", 0)

    try:
        gpu_ctx.set_option("blas_cones", 1)
        i0, img0, _ = two_frames(gpu_ctx, c3(), 0, toggle)
        gpu_ctx.set_option("blas_cones", 1)
        i1, img1, rebuilt = two_frames(gpu_ctx, c3(), 1, toggle)
        assert [i["tile_entry"] for i in i1] == [1, 1] and [i["cones"] for i in i1] == [1, 0] and rebuilt == 1, (i1, rebuilt)
        for a, b in zip(img1, img0):
            assert same(a, b)
    finally:
        restore(gpu_ctx)


def test_spheres_switch_it_off(gpu_ctx):
    sc = scenes.mixed_test_scene(96, 64)
    assert len(sc.spheres) > 0
    try:
        t0, c0, i0, _ = trace(gpu_ctx, sc, 2, 0)
        t1, c1, i1, _ = trace(gpu_ctx, sc, 2, 1)
        assert i0["tile_entry"] == 0 and i1["tile_entry"] == 0, (i0, i1)
        assert same(t1, t0) and same(c1, c0)
    finally:
        restore(gpu_ctx)


def test_counters_equal_the_oracles(gpu_ctx):
    sc = c3()
    sc.num_bounces = 4
    try:
        gpu_ctx.set_option("tile_entry", 1)
        gpu_ctx.set_option("count_stats", 1)
        m = RayTraceMaster(gpu_ctx, sc)
        gpu_ctx.reset_counters()
        m.OnRenderImage()
        got = m._target.GetPixels()
        gc = gpu_ctx.counters()
        info = gpu_ctx.launch_info()
        o = pyoracle.Oracle(sc)
        o.set_blas(*gpu_ctx.read_scene_blas(len(sc.mesh_objects))[:3])
        m.OnDisable()
        assert info["count_stats"] == 1 and info["tile_entry"] == 0 and info["kernel"].startswith("k_sched<true, "), info
        ref, oc = o.render(mode=1, threads=8, counters=True)
        assert same(got, ref)
        for k in ("rays", "tlas_nodes", "blas_nodes", "tri_tests", "sphere_tests", "hit_tri", "hit_sphere", "hit_ground", "hit_sky"):
            assert gc[k] == oc[k], (k, gc[k], oc[k])
    finally:
        restore(gpu_ctx)


def leaf_ranges(nodes, code):
    """[first, end) leaf-order triangle ranges below a node code of the device's tree"""
    out, todo = [], [int(code)]
    kids = np.ascontiguousarray(nodes[:, 12:14]).view(np.int32)
    while todo:
        c = todo.pop()
        if c == DONE:
            continue
        if c < 0:
            u = (~c) & 0xFFFFFFFF
            out.append((u >> 3, (u >> 3) + (u & 7) + 1))
        else:
            todo += [int(kids[c, 0]), int(kids[c, 1])]
    return out


@pytest.mark.parametrize("view", ["C3", "close-up"])
def test_no_ray_of_a_tile_hits_outside_its_list(gpu_ctx, view):
    sc = c3() if view == "C3" else c3(position=(0.0, 2.4, -7.3))
    W, H = sc.width, sc.height
    try:
        gpu_ctx.set_option("tile_entry", 1)
        m = RayTraceMaster(gpu_ctx, sc)
        m.OnRenderImage()
        m._target.GetPixels()
        assert gpu_ctx.launch_info()["tile_entry"] == 1
        table, _ = gpu_ctx.read_tile_entry()
        nodes, tri_index, _ = gpu_ctx.read_scene_blas(1)[:3]
        assert table.shape == ((H + 7) // 8, (W + 7) // 8, 8)
        # sample positions per tile: the corners of [8 tx, 8 tx + 9] x [8 ty, 8 ty + 9] (pixel + rand + offset, both in [0, 1]) and 32 random ones
        rng = np.random.default_rng(5)
        ty, tx = np.mgrid[0:table.shape[0], 0:table.shape[1]]
        fx = np.concatenate([np.array([0.0, 9.0, 0.0, 9.0]), rng.uniform(0, 9, 32)])
        fy = np.concatenate([np.array([0.0, 0.0, 9.0, 9.0]), rng.uniform(0, 9, 32)])
        sx = (8 * tx[..., None] + fx).reshape(-1)
        sy = (8 * ty[..., None] + fy).reshape(-1)
        tile = np.repeat(np.arange(table.shape[0] * table.shape[1]), len(fx))
        c2w = np.asarray(sc.camera_to_world, np.float64).reshape(4, 4).T
        invp = np.asarray(sc.camera_inverse_projection, np.float64).reshape(4, 4).T
        uv = np.stack([sx / W * 2 - 1, sy / H * 2 - 1, np.zeros_like(sx), np.ones_like(sx)])
        d = c2w[:3, :3] @ (invp @ uv)[:3]
        d = (d / np.linalg.norm(d, axis=0)).T
        o = np.broadcast_to(c2w[:3, 3], d.shape)
        hits = gpu_ctx.ray_query(o.astype(np.float32), d.astype(np.float32))
        m.OnDisable()
        slot_of = {int(s): k for k, s in enumerate(tri_index)}              # index slot -> leaf-order position
        flat = table.reshape(-1, 8)
        allowed = {}
        n_tri = 0
        for r in np.flatnonzero(hits["kind"] == 3):
            t = int(tile[r])
            if t not in allowed:
                allowed[t] = [rg for code in flat[t] for rg in leaf_ranges(nodes, code)]
            k = slot_of[int(hits["primitive"][r])]
            assert any(a <= k < b for a, b in allowed[t]), f"tile {t}: a ray hits leaf-order triangle {k}, outside the list {flat[t]}"
            n_tri += 1
        assert n_tri > len(tile) // 20, n_tri                   # (the mesh covers more than a twentieth of either view: the check is not vacuous)
    finally:
        restore(gpu_ctx)
