"""GPU: the default trace kernel (kernel_mode 3) and the shared-service kernel (mode 5) on BOTH sides of every size at which their LDS
layout switches (csrc/frame_batch.cpp configure_sched_at, csrc/scene_prep.cpp prepare_scene, the prologue of k_sched in csrc/kernels.hip):

    listed FRONT            n_meshes <= 12                          masked FRONT (walk table in LDS)   mesh heap <= 31 nodes
    mesh heap + roots       heap <= 256 nodes, <= 256 MeshObjects   sphere heap + spheres              heap <= 256 nodes, <= 256 spheres
    small-triangle copy     1 .. 64 single-leaf triangles           FRONT at all                       n_meshes > 1
    per-lane object-level stack   levels(larger heap) + 1; under the masked FRONT the sphere heap's alone

Each case renders a scene of tests/threshold_scenes.py (held to its sizes and to being worth rendering by tests/test_threshold_scenes.py):
pixels bit for bit against the oracle on its own BVH and against its literal brute force, traversal counters against the oracle on the
product's tree, and the layout urt_debug_launch_info reports against LITERAL expectations — which tables are in LDS, which FRONT ran, how
deep the object-level stack is.  Then every other kernel on the far sides, the query kernels (which size their LDS from the scene's stack
depth, not the frame kernel's), and a live scene that crosses a threshold and comes back."""
import numpy as np
import pytest

import threshold_scenes as T
from oracle import pyoracle
from unityraytracer_amd import Context, RayTraceMaster
from test_gpu_aov import assert_matches_queries, camera_rays
from test_gpu_parity import assert_same, oracle_for
from test_gpu_radiance_query import all_pixels, bits
from test_gpu_ray_query import assert_matches_oracle, oracle_trace

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "tlas_nodes", "blas_nodes", "tri_tests", "sphere_tests", "hit_tri", "hit_sphere", "hit_ground", "hit_sky", "pixels")
MESH, SPHERE, SMALL, WALK = 1, 2, 4, 8          # urt_launch_info.lds_tables
DEFAULTS = {"kernel_mode": 3, "count_stats": 0, "front_list": -1, "lds_tlas": 1, "blas_leaf_max": 2, "frames_per_launch": 0}


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    """A context of this module's own: no buffers of another module's scene stay bound (a scene without meshes binds no mesh buffers),
    and its options start at their defaults."""
    with Context(gpu_ctx.device) as c:
        yield c
        c.set_option("blas_leaf_max", 2)            # (process-wide)


_refs = {}


def reference(ctx, name):
    """(scene, pixels, counters) of case `name`, computed once: the oracle's frame on its own BVH, which must equal its literal brute
    force (RS:243: every triangle of every MeshObject) and its frame on the product's tree; the counters are that last frame's."""
    if name not in _refs:
        sc = T.CASES[name][0]()
        o = pyoracle.Oracle(sc)
        if len(sc.mesh_objects):
            o.build_own_blas()
        own = o.render(mode=1, threads=8)
        assert_same(o.render(mode=0, threads=8), own, f"{name}: the oracle's brute force vs its own BVH")
        ctx.set_option("blas_leaf_max", T.CASES[name][6])          # debug_build_blas follows the process-wide leaf size
        try:
            prod, oc = oracle_for(sc).render(mode=1, threads=8, counters=True)
        finally:
            ctx.set_option("blas_leaf_max", 2)
        assert_same(prod, own, f"{name}: the oracle on the product's tree vs its own BVH")
        own.setflags(write=False)
        _refs[name] = (sc, own, oc)
    return _refs[name]


def render(ctx, name, mode=3, **options):
    """One frame of case `name` with count_stats -> (pixels, counters, launch info).  Options are restored."""
    sc = T.CASES[name][0]()
    m = None
    try:
        ctx.set_option("blas_leaf_max", T.CASES[name][6])
        for k, v in options.items():
            ctx.set_option(k, v)
        ctx.set_option("kernel_mode", mode)
        ctx.set_option("count_stats", 1)
        ctx.reset_counters()
        m = RayTraceMaster(ctx, sc)
        m.OnRenderImage()
        img = m._target.GetPixels()
        return img, ctx.counters(), ctx.launch_info()
    finally:
        if m is not None:
            m.OnDisable()
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


def assert_is_the_oracle(ctx, name, img, gc, what):
    sc, ref, oc = reference(ctx, name)
    assert_same(img, ref, what)
    for k in COUNTERS:
        assert gc[k] == oc[k], (what, k, gc[k], oc[k])
    assert gc["watchdog_trips"] == 0, what


# ---- 2a. both sides of every switch, and the layout that ran ---------------------------------------------------------------------
# (case, options, front_mode, lds_tables, tlas_stack or None).  Literal values, read off configure_sched_at; nothing here is computed
# from the library.  Rows 12 and 13 MeshObjects with "front_list" 2: 12 and 13 objects make a heap of ceil(log2 n) + 1 = 5 levels
# (31 nodes), and the stack is levels + 1 = 6 (scene_prep.cpp pack_scene_tables), as 63 nodes give 7 and 255 give 9.  Quads alone have
# no triangle-BVH node, so there is no top of the forest for FRONT to walk and front_mode is 0 (`top_in_front && P.top_nodes > 0`); with
# one multi-leaf MeshObject among them it is 1.  For the same reason the masked cases of the small-triangle copy carry one icosphere.
ROWS = [
    ("m1", {}, 0, MESH, 2),                                  # one MeshObject: no FRONT at all, its 1-node heap and root in LDS
    ("m2", {}, 3, WALK, 2), ("m3", {}, 3, WALK, 2), ("m4", {}, 3, WALK, 2), ("m5", {}, 3, WALK, 2),
    ("m12", {}, 3, WALK, 2),
    ("m12", {"front_list": 2}, 2, MESH, 6),                  # the last listed size
    ("m13", {"front_list": 2}, 1, MESH, 6),                  # one more: the plain FRONT
    ("m13", {}, 3, WALK, 2),
    ("m16", {}, 3, WALK, 2),                                 # 31 nodes: the last masked size
    ("m17", {}, 1, MESH, 7),                                 # 63 nodes
    ("m16+s129", {}, 3, WALK, 10),                           # masked: the stack is the sphere heap's (511 nodes, 9 levels), which is not in LDS
    ("m128", {}, 1, MESH, 9),                                # 255 nodes
    ("m129", {}, 1, 0, 10),                                  # 511 nodes: heap and roots stay in global memory
    ("s128", {}, 0, SPHERE, 9),
    ("s129", {}, 0, 0, 10),
    ("m3+s257", {}, 3, WALK, 11),                            # 1,023 sphere-heap nodes
    ("fans8+big", {}, 3, WALK | SMALL, None),                # 64 single-leaf triangles: the last LDS size, masked form of the copy
    ("fans9+big", {}, 3, WALK, None),                        # 72: dropped, every small_first is -1
    ("quads32", {}, 0, MESH | SMALL, None),                  # 64 again, the lds_mesh form of the copy; front_mode 0, see above
    ("quads33", {}, 0, MESH, None),                          # 66
    ("quads32+big", {}, 1, MESH | SMALL, None),              # small_first holds -1 between real entries
]
ROW_IDS = [name + "".join(f",{k}={v}" for k, v in opts.items()) for name, opts, _, _, _ in ROWS]


@pytest.mark.parametrize("row", range(len(ROWS)), ids=ROW_IDS)
def test_each_side_renders_the_oracle_in_the_layout_its_size_selects(ctx, row):
    name, opts, front_mode, tables, tlas_stack = ROWS[row]
    img, gc, info = render(ctx, name, 3, **opts)
    print(f"{ROW_IDS[row]}: front_mode {info['front_mode']} lds_tables {info['lds_tables']} tlas_stack {info['tlas_stack']} "
          f"top_nodes {info['top_nodes']} lds_bytes {info['lds_bytes']} {info['kernel']}")
    assert_is_the_oracle(ctx, name, img, gc, ROW_IDS[row])
    assert info["kernel_mode"] == 3
    assert (info["front_mode"], info["lds_tables"]) == (front_mode, tables), info
    if tlas_stack is not None:
        assert info["tlas_stack"] == tlas_stack, info
    again = render(ctx, name, 3, **opts)[2]
    assert again["lds_bytes"] == info["lds_bytes"] and again["lds_tables"] == tables


# every pair of neighbouring cases whose table bits differ, by case id
PAIRS = [("m1", "m2"), ("m12", "m12,front_list=2"), ("m16", "m17"), ("m128", "m129"), ("s128", "s129"), ("fans8+big", "fans9+big"),
         ("quads32", "quads33")]


@pytest.mark.parametrize("a, b", PAIRS)
def test_lds_size_follows_the_tables(ctx, a, b):
    """Across every pair whose table bits differ, so does the workgroup's LDS."""
    ra, rb = ROWS[ROW_IDS.index(a)], ROWS[ROW_IDS.index(b)]
    assert ra[3] != rb[3]
    ia, ib = render(ctx, ra[0], 3, **ra[1])[2], render(ctx, rb[0], 3, **rb[1])[2]
    assert (ia["lds_tables"], ib["lds_tables"]) == (ra[3], rb[3]) and ia["lds_bytes"] != ib["lds_bytes"], (ia, ib)


# ---- 2b. every kernel on the far sides -------------------------------------------------------------------------------------------
FAR = ["m13", "m17", "m129", "s129", "m16+s129", "fans9+big", "quads33"]


@pytest.mark.parametrize("name", FAR)
def test_every_kernel_on_the_far_side(ctx, name):
    for mode in (0, 1, 2, 4, 5):
        img, gc, info = render(ctx, name, mode)
        assert_is_the_oracle(ctx, name, img, gc, f"{name}, kernel_mode {mode}")
        if mode == 5:
            assert info["front_mode"] != 3, info                  # the shared-service kernel has no masked FRONT
    img, gc, info = render(ctx, name, 3, lds_tlas=0)
    assert_is_the_oracle(ctx, name, img, gc, f"{name}, lds_tlas 0")
    assert info["lds_tables"] == 0 and info["front_mode"] != 3, info


# ---- 2c. the query kernels take their stack depth from the scene ---------------------------------------------------------------------
@pytest.mark.parametrize("name, frame_stack, kind", [("s129", 10, 2), ("m16+s129", 10, 2), ("m16", 2, 3)])
def test_queries_size_their_stack_from_the_scene(ctx, name, frame_stack, kind):
    """129 spheres: a 10-entry object-level stack, in the frame kernel and in the query kernels.  16 MeshObjects: the frame kernel walks them
    with masks and keeps a 2-entry stack, while the query kernels walk the 31-node heap with the scene's 6 entries — the case where the two
    depths differ; with 129 spheres beside them both are 10."""
    sc, ref, _ = reference(ctx, name)
    w, h = sc.width, sc.height
    m = RayTraceMaster(ctx, sc)
    try:
        m.OnRenderImage()
        img = m._target.GetPixels()
        assert_same(img, ref, name)
        assert ctx.launch_info()["tlas_stack"] == frame_stack
        xy = all_pixels(w, h)
        got = ctx.radiance_query_pixels(xy, 1, 4)                 # the uniforms of that frame are still bound
        assert np.array_equal(bits(got), bits(img[xy[:, 1], xy[:, 0]]))
        O, D = camera_rays(sc, w, h)
        hits = ctx.ray_query(O.reshape(-1, 3), D.reshape(-1, 3))
        assert_matches_oracle(hits, oracle_trace(pyoracle.Oracle(sc), O.reshape(-1, 3), D.reshape(-1, 3), mode=0), name)
        assert (hits["kind"] == kind).mean() > 0.2
        assert_matches_queries(ctx, ctx.render_aov_arrays(w, h), O, D, name)
    finally:
        m.OnDisable()


# ---- 2d. a live scene crosses a threshold and comes back ---------------------------------------------------------------------------
@pytest.mark.parametrize("fpl", [0, 1])
@pytest.mark.parametrize("near, far, t_near, t_far", [("s128", "s129", SPHERE, 0), ("m16", "m17", WALK, MESH), ("quads32", "quads33", MESH | SMALL, MESH)])
def test_crossing_a_threshold_between_frames(ctx, near, far, t_near, t_far, fpl):
    """One RayTraceMaster: 2 frames on the near side, the buffers re-created for the far side (the counts change: a full preparation,
    capacities kept), 2 frames, back, 2 frames.  After every step the last frame is the one a fresh context renders from that scene at
    that frame index, and the layout has followed."""
    scs = {k: T.CASES[k][0]() for k in (near, far)}
    m = None
    try:
        ctx.set_option("frames_per_launch", fpl)
        m = RayTraceMaster(ctx, scs[near])
        for step, (side, tables) in enumerate(((near, t_near), (far, t_far), (near, t_near))):
            m.scene = scs[side]
            m.RebuildTrees()
            m.OnRenderImage(); m.OnRenderImage()
            img = m._target.GetPixels()
            assert ctx.launch_info()["lds_tables"] == tables, (step, side, ctx.launch_info())
            with Context(ctx.device) as fresh:
                f = RayTraceMaster(fresh, scs[side])
                f._frame = m._frame - 1
                f.OnRenderImage()
                want = f._target.GetPixels()
                f.OnDisable()
            assert_same(img, want, f"step {step}: {side} at frame {m._frame - 1}, frames_per_launch {fpl}")
            assert (img[..., :3] > 0).any(axis=2).mean() > 0.5
    finally:
        if m is not None:
            m.OnDisable()
        ctx.set_option("frames_per_launch", 0)
