"""GPU: the refill of the scheduled trace kernel (csrc/kernels.hip k_sched) works out what is the same for every lane once — a slot's
tile -> pixel origin per tile on wave-uniform values (csrc/frame_device.h wg_fetch_pixels), and the seed-only half of a new pixel's first
two rand() draws and the camera ray's origin per frame, on the host, into the launch's frame table (csrc/frame_derived.h,
camera_ray_frame).  Per pixel the operations and their operands are the same, so at every case below, kernel mode 3, with the hand-out
per workgroup ("handout" 1) and per wave (0):
    the last traced frame and the accumulated image == the oracle, bit for bit, and the watchdog counter stays 0.
The sky is 64 x 32 throughout.  Cases:
  * frames of 1 x 1, 65 x 3, 7 x 130, 96 x 64, 57 x 16 and 41 x 24: ragged right and top edges, fewer tiles than shards, one tile per
    frame, tiles_x a power of two (1, 8) and not (9, 12, 6);
  * launches of 1, 2, 4 and 64 frames, frame after frame ("frame_group" 1: refills straddle a tile and a frame boundary at once) and
    interleaved (auto);
  * run lengths 1, 8, 24 and 4096, top-down tile order, both ranks of a two-rank strip split (row_stride 2, first_group_row 0 / 1);
  * _Seed 0, 1e-31 (below f_div_const's range: the divider path), 100.25 and 3e38 on a 16 x 16 frame;
  * three rays per pixel (the seed carried behind the table-fed first ray), the blob with spheres (the general object-level walk);
  * SHADE trips of ground-plane hits alone and of ground and triangle hits together (what a vote on the ground plane's constant tangent
    frame would split: profiles/r25_logs/ground_frame_vote.patch, measured and not kept — these cases guard a second attempt).  The
    ground plane's material is the reference's own, hard-coded and purely diffuse (RS:164-170), so the four kinds of material — purely diffuse, purely specular, both chances non-zero, a roulette that ends most paths — go onto the
    blob, on a scene whose waves see only ground and sky (the blob stands behind the camera) and on one where ground and triangle hits
    share waves; and a scene with no object at all;
  * material tables (spheres + mesh objects + the ground plane) of 2 and 6 entries, of 7, 8 and 9 (the blob with 5, 6 and 7 spheres:
    one below, at and one above the 8 entries up to which profiles/r25_logs/lds_materials.patch copies the table to LDS — measured and
    not kept; the cases pass with the patch applied and without it) and of 301 (scenes.many_meshes_scene);
  * with count_stats the nine counters equal the oracle's (the first scene of the list, the blob with spheres, a table at the
    threshold, one above it, the 301 materials)."""

import numpy as np
import pytest

from oracle import pyoracle
from test_gpu_handout import NINE, frames_of, oracle_frames, restore, scene
from test_gpu_front_fuse import blobs, differing, same
from unityraytracer_amd import RayTraceMaster, scenes, strips

pytestmark = pytest.mark.gpu


def check(ctx, name, frames=4, opts=None, rank=0, world=1, front=0):
    sc, scene_opts, scene_front = scene(name)
    front = scene_front if front == 0 else front
    what = f"{name} x{frames} {opts or {}} rank {rank}/{world}"
    try:
        for k, v in {**scene_opts, **(opts or {})}.items():
            ctx.set_option(k, v)
        img = acc = None
        for handout in (1, 0):
            t, c, info, tree, g = frames_of(ctx, sc, frames, handout, rank, world)
            assert info["kernel_mode"] == 3 and (front is None or info["front_mode"] == front) and info["n_frames"] == frames, (what, info)
            assert info["kernel"].startswith("k_sched<false, "), (what, info)
            assert (info["handout"] > 0) == (handout == 1), (what, info)
            if img is None:
                img, acc = oracle_frames(name, sc, tree, frames, rank, world)
            assert same(t, img) and same(c, acc), f"{what}: handout {handout} differs from the oracle in {differing(t, img)} / {differing(c, acc)} pixels"
            assert g["watchdog_trips"] == 0, what
        return info
    finally:
        restore(ctx)


@pytest.mark.parametrize("name", ["1x1", "65x3", "7x130", "96x64", "57x16", "41x24"])
def test_frame_shapes(gpu_ctx, name):
    check(gpu_ctx, name, 4)


@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("frames", [1, 2, 4, 64])
def test_frames_per_launch(gpu_ctx, frames, group):
    """41 x 24 = 18 tiles of 6 per row; with frame_group 1 a reservation runs on from one frame into the next (64: all frames interleaved, what auto takes)"""
    i = check(gpu_ctx, "41x24", frames, {"frames_per_launch": frames, "xcd_run": 8, "frame_group": group})
    assert i["frame_group"] == min(group, frames), i


@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("run", [1, 8, 24, 4096])
def test_run_lengths(gpu_ctx, run, group):
    i = check(gpu_ctx, "96x64", 4, {"xcd_run": run, "frame_group": group})
    assert i["xcd_run"] == run, i


@pytest.mark.parametrize("opts", [{"tile_order": 1}, {"tile_order": 1, "frame_group": 1, "xcd_run": 8}])
def test_top_down_order(gpu_ctx, opts):
    check(gpu_ctx, "96x64", 4, opts)


@pytest.mark.parametrize("rank", [0, 1])
def test_strips_of_a_two_rank_split(gpu_ctx, rank):
    assert strips.strip_row_ranges(64, rank, 2)
    check(gpu_ctx, "96x64", 4, {"xcd_run": 2}, rank=rank, world=2)


@pytest.mark.parametrize("seed", [0.0, 1e-31, 100.25, 3e38])
def test_seeds(gpu_ctx, seed):
    """frame 0 takes the scene's own _Seed: the table's a0 / a1 come from it through both paths of f_div_const"""
    sc = scenes.config3(16, 16, slices=24, stacks=20, sky=scenes.make_sky(64, 32))
    sc.seed = float(np.float32(seed))
    try:
        ref = None
        for handout in (1, 0):
            gpu_ctx.set_option("handout", handout)
            gpu_ctx.reset_counters()
            m = RayTraceMaster(gpu_ctx, sc)
            try:
                m.OnRenderImage()
                t = m._target.GetPixels()
                info = gpu_ctx.launch_info()
                assert info["kernel_mode"] == 3 and info["n_frames"] == 1 and info["kernel"].startswith("k_sched<false, "), info   # through the frame table
                assert (info["handout"] > 0) == (handout == 1), info
                tree = gpu_ctx.read_scene_blas(len(sc.mesh_objects))[:3]
            finally:
                m.OnDisable()
            if ref is None:
                o = pyoracle.Oracle(sc)
                o.set_blas(*tree)
                o.set_frame(sc.pixel_offset, sc.seed)
                ref = o.render(mode=1, threads=8)
            assert same(t, ref), f"_Seed {seed}: handout {handout} differs from the oracle in {differing(t, ref)} pixels"
            assert gpu_ctx.counters()["watchdog_trips"] == 0
    finally:
        restore(gpu_ctx)


@pytest.mark.parametrize("name", ["three-rays", "C3-spheres"])
def test_carried_seed_and_general_walk(gpu_ctx, name):
    check(gpu_ctx, name, 4)


MATERIALS = {"diffuse": ((0.8, 0.6, 0.4), (0, 0, 0), (0, 0, 0), 0.2), "specular": ((0, 0, 0), (0.9, 0.8, 0.7), (0, 0, 0), 0.9),
             "both": ((0.5, 0.4, 0.3), (0.3, 0.3, 0.3), (0, 0, 0), 0.6), "roulette": ((0.3, 0.1, 0.2), (0.1, 0.05, 0.1), (0.4, 0.3, 0.2), 0.5)}


def shading_scene(name):
    """"<material>-<where>": one blob of that material in view ("mixed": ground and triangle hits share waves) or behind the camera
    ("ground": the waves see ground and sky); "empty": no object at all; "many": 301 materials"""
    from test_gpu_handout import _scenes
    if name not in _scenes:
        if name == "empty":
            sc = scenes.Scene("empty", 96, 64, 8, 1, sky=scenes.make_sky(64, 32))
        elif name == "many":
            sc = scenes.many_meshes_scene(64, 40, sky=scenes.make_sky(64, 32))
        elif name.startswith("mats"):                           # the blob, the ground plane and n - 2 spheres
            sc = blobs(96, 64, [(0.0, -4.0, 2.2)], n_spheres=int(name[4:]) - 2)
        else:
            mat, where = name.split("-")
            sc = blobs(96, 64, [(0.0, -4.0 if where == "mixed" else -40.0, 2.2)], material=scenes._params(*MATERIALS[mat]))
        _scenes[name] = (sc, {}, None)
    return _scenes[name]


@pytest.mark.parametrize("where", ["ground", "mixed"])
@pytest.mark.parametrize("mat", sorted(MATERIALS))
def test_ground_and_mesh_materials(gpu_ctx, mat, where):
    name = f"{mat}-{where}"
    shading_scene(name)
    check(gpu_ctx, name, 4, front=None)


def test_nothing_but_ground_and_sky(gpu_ctx):
    shading_scene("empty")
    check(gpu_ctx, "empty", 4, front=None)


LDS_MATERIALS = 8                                               # kLdsMaterials of profiles/r25_logs/lds_materials.patch


@pytest.mark.parametrize("name", ["96x64", "C3-spheres", "mats7", "mats8", "mats9", "many"])
def test_material_tables(gpu_ctx, name):
    """2 materials (blob + ground), 6 (four spheres, blob, ground), one below, at and one above the LDS threshold, and 301"""
    if name not in ("96x64", "C3-spheres"):
        shading_scene(name)
    sc = scene(name)[0]
    assert len(sc.spheres) + len(sc.mesh_objects) + 1 == {"96x64": 2, "C3-spheres": 6, "mats7": LDS_MATERIALS - 1, "mats8": LDS_MATERIALS,
                                                          "mats9": LDS_MATERIALS + 1, "many": 301}[name]
    check(gpu_ctx, name, 2, front=None)


@pytest.mark.parametrize("name", ["1x1", "C3-spheres", "mats8", "mats9", "many"])
def test_counters_equal_the_oracles(gpu_ctx, name):
    if name not in ("1x1", "C3-spheres"):
        shading_scene(name)
    sc, opts, front = scene(name)
    try:
        for k, v in opts.items():
            gpu_ctx.set_option(k, v)
        gpu_ctx.set_option("count_stats", 1)
        t, _, info, tree, gc = frames_of(gpu_ctx, sc, 1, 1)
        assert info["count_stats"] == 1 and (front is None or info["front_mode"] == front) and info["handout"] > 0 and info["kernel"].startswith("k_sched<true, "), info
        o = pyoracle.Oracle(sc)
        o.set_blas(*tree)
        o.set_frame(scenes.frame_uniforms(0)[:2], scenes.frame_uniforms(0)[2])
        ref, oc = o.render(mode=1, threads=8, counters=True)
        assert same(t, ref)
        for k in NINE:
            assert gc[k] == oc[k], (k, gc[k], oc[k])
        assert gc["watchdog_trips"] == 0
    finally:
        restore(gpu_ctx)
