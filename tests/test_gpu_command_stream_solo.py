"""GPU: program order in the solo world (the "solo" profile of tests/command_stream.py): ONE MeshObject and no sphere, so the trace launches
are the plain single-mesh form of k_sched — front_fuse 2, the normal cones, the LDS top and the tile entry table of option "tile_entry"
(csrc/frame_batch.cpp tile_entry_for_launch: one table per context, cached by camera, size and node contents, rebuilt on whichever
stream misses behind the readers on the other streams) — with urt_motion_blur among the image calls and, in some runs, option
"prepare_device": every full preparation then reads the device mirrors the un-waited skins, morphs, SetDataDevice and ring uploads go to.

The world.  The blob is tessellated 20 x 15 (cs.SOLO_BLOB: 282 vertices, 560 triangles, a triangle BVH of depth 11).  What the table of
CAMERA_POSITIONS[0] at 64 x 40 held on an MI355X is in test_the_solo_world_is_what_the_issue_asks_for.

What the pixel comparison can and cannot decide.  Two mutations of csrc/frame_batch.cpp were run against the directed protocols by hand
(DESIGN.md section 7): without nodes_epoch in the table's key every protocol still passes — every scene preparation, the in-place ones
included, bumps scene_epoch, which is in the key too; with both epochs out protocol 2 fails by its builds count and protocol 3 by its
pixels — and without the wait for te_used[] of the other streams they pass as well: at
these sizes the launch that reads the old table has ended before the host has submitted the rebuild.  The protocols hold what the
library reports (which launches used a table, how many were built, what the table lists) and the pixels; they do not prove the wait.

Fuzz: the baseline is the undeferred run WITHOUT the table; it equals the sequential model bit for bit (the denoised image within
urt_denoise's bound).  Every deferring configuration with the table forced, two with the table on auto, and two with refit 0 and
prepare_device 1 equal the baseline bit for bit, the ray counter included.  The reach of the seed set is held by
tests/test_command_stream_model.py.

Directed protocols: each runs once per configuration and none reruns; each asserts that it shows something."""
import numpy as np
import pytest

import command_stream as cs
from test_gpu_command_stream import DEFERRING, SHAPE, UNDEFERRED, launches, protocol

pytestmark = pytest.mark.gpu

DONE = -2 ** 31                                                  # the padding of a tile's entry list
W = cs.dynamic_world(world="solo")
LO, HI = W["span"]
NV = len(W["rest_v"])
TABLE_ON, TABLE_AUTO, TABLE_OFF = dict(tile_entry=1), dict(tile_entry=-1), dict(tile_entry=0)
DEVICE_FED = dict(refit=0, prepare_device=1, tile_entry=1)
PREPARES = ("frame", "dispatch", "aov", "aov_into", "aov_low", "ray_query", "radiance_query", "radiance_pixels", "resample", "ray_query_async",
            "radiance_async", "present_tm")
VERTEX_EDITS = cs.SOLO_VERTEX_WRITES + ("deform",)


def check(what, program, got, want):
    d = cs.first_difference(got, want, radiance=True)
    if d is not None:
        upto, text = d
        raise AssertionError(f"{what}: {text}\nops{'' if upto is None else ' up to it'}:\n{cs.describe(program, upto)}")


def run(ctx, program, cfg, options=None, profile="solo", **kw):
    return cs.run_gpu(ctx, program, *cfg, profile=profile, options=options, **kw)


def used_the_table(got, program):
    """launch_info()["tile_entry"] wherever the run asked, behind the program's first frame (before it the last launch is an earlier run's)."""
    first = min(i for i, op in enumerate(program) if op[0] in ("frame", "dispatch"))
    return [info["tile_entry"] for i, info in got[3] if i > first or i == -1]


def frames_prepared_behind_a_vertex_write(program):
    """Frames that are the first preparing op behind a vertex write (one preparation serves every write in front of it): with refit 0
    each of them ends in a full preparation."""
    n, dirty = 0, False
    for op in program:
        edit = op[1] if op[0] == "device_heap" else op
        if edit[0] in VERTEX_EDITS:
            dirty = True
        elif op[0] in PREPARES:
            n += dirty and op[0] == "frame"
            dirty = False
    return n


def download_probe(ctx):
    """Records, after every op, the synchronising downloads of V, NB and the index buffer so far (buffer_state neither submits nor waits)."""
    def probe(i, op, m, pw):
        probe.seen.append([ctx.buffer_state(b)["downloads"] for b in (pw.V, pw.NB, m._indexBuffer)])
        v = ctx.buffer_state(pw.V)
        probe.stale.append((v["stale_first"], v["stale_last"]))
    probe.seen, probe.stale = [], []
    return probe


def downloads_nobody_asked_for(program, seen, stale):
    """[(op index, op, growth of the downloads of V, NB, the indices)] between the first and the last frame, over the ops that have no
    download of their own.  The ops that have one: get_buffer of that buffer, and a ranged host SetData into V (set_host, wrapped or
    not) that would SPLIT the range in which the device mirror is newer — include/urt.h: the part behind the written elements comes
    down first.  stale[i]: that range of V after op i (first > last: none); a deform writes the whole span and splits nothing."""
    frames = [i for i, op in enumerate(program) if op[0] == "frame"]
    out = []
    for i in range(frames[0] + 1, frames[-1] + 1):
        op = program[i][1] if program[i][0] == "device_heap" else program[i]
        s0, s1 = stale[i - 1]
        splits = op[0] == "set_host" and s0 <= s1 and s0 < op[1] and op[1] + op[2] - 1 < s1
        own = [splits or op[:2] == ("get_buffer", "V"), op[:2] == ("get_buffer", "NB"), False]
        grown = [b - a for a, b in zip(seen[i - 1], seen[i])]
        if any(g and not o for g, o in zip(grown, own)):
            out.append((i, program[i], grown))
    return out


def test_the_solo_world_is_what_the_issue_asks_for(gpu_ctx):
    """20 x 15 slices x stacks (282 vertices, 560 triangles, a triangle BVH of depth 11).  The table of CAMERA_POSITIONS[0] at 64 x 40
    (8 x 5 tiles of 8 entries) on an MI355X: 37 empty tiles, 3 listed ones, each of 2 entries or more (at most 4), whose first entries are
    the codes -3697 (a leaf), 2 and 7 — none starts at the root (profiles/r31_logs/solo_replay_times.log)."""
    sc = cs.make_scene(world="solo")
    assert len(sc.mesh_objects) == 1 and len(sc.spheres) == 0 and len(sc.sphere_bvh) == 0 and sc.num_rays == 1
    assert (LO, HI) == (0, NV - 1) == cs.blob_span(sc), "the blob's span is not the whole vertex list"
    mixed = cs.make_scene()
    assert np.array_equal(sc.mesh_objects["localToWorldMatrix"][0], mixed.mesh_objects["localToWorldMatrix"][0]) and np.array_equal(sc.sky, mixed.sky)
    before = gpu_ctx.read_tile_entry()[1]
    got = run(gpu_ctx, [("frame", None), ("frame", None), ("get", "T0")], UNDEFERRED, TABLE_ON)
    info = got[3][-1][1]
    table, builds = gpu_ctx.read_tile_entry()
    assert info["tile_entry"] == 1 and info["front_mode"] == 0 and info["blas_stack"] >= 8 and builds == before + 1, (info, builds, before)
    from unityraytracer_amd.unity_api import debug_build_blas
    _, _, roots, _, depth = debug_build_blas(sc.mesh_objects, sc.vertices, sc.indices)
    counts = (table != DONE).sum(axis=2)
    first = table[..., 0][counts > 0]
    values, n = np.unique(first, return_counts=True)
    print(f"solo world: tessellation {cs.SOLO_BLOB}, BVH depth {depth}; table {table.shape}: {int((counts == 0).sum())} empty tiles, "
          f"{int((counts >= 2).sum())} tiles of 2 entries or more (at most {int(counts.max())}), the root is {int(roots[0])}, first entries {dict(zip(values.tolist(), n.tolist()))}")
    assert depth > 8 and table.shape == (5, 8, 8)
    assert (counts == 0).any() and (counts >= 2).any(), counts
    assert (first != roots[0]).any() and len(values) >= 2, ("every listed tile starts at the root: the table prunes nothing", int(roots[0]), values)


@pytest.mark.parametrize("seed", range(24))
def test_random_solo_programs_keep_program_order(gpu_ctx, seed):
    program = cs.make_program(seed, profile="solo")
    model = cs.run_model(program, profile="solo")
    assert any(op[0] == "frame" for op in program)
    plain = run(gpu_ctx, program, UNDEFERRED, TABLE_OFF)
    check(f"seed {seed}, configuration {UNDEFERRED} without the table against the model", program, plain, model)
    assert plain[2]["watchdog_trips"] == 0 and not any(used_the_table(plain, program))
    runs = [(cfg, TABLE_ON) for cfg in DEFERRING] + [((1, 2), TABLE_AUTO), ((0, 1), TABLE_AUTO), (UNDEFERRED, DEVICE_FED), ((0, 2), DEVICE_FED)]
    for cfg, options in runs:
        probe = download_probe(gpu_ctx)
        prepared = gpu_ctx.prepare_stats()["device"]
        got = run(gpu_ctx, program, cfg, options, probe=probe)
        what = (seed, cfg, options)
        check(f"seed {seed}, configuration {cfg} with {options} against the baseline", program, got, plain)
        assert got[2]["rays"] == plain[2]["rays"] and got[2]["dispatches"] == plain[2]["dispatches"], (what, got[2], plain[2])
        assert got[2]["watchdog_trips"] == 0, what
        if options["tile_entry"] == 1:
            assert 1 in used_the_table(got, program), (what, "no launch_info() of the run shows the table in use", got[3])
        if options is DEVICE_FED:
            want = frames_prepared_behind_a_vertex_write(program)
            grown = gpu_ctx.prepare_stats()["device"] - prepared
            assert grown >= max(want, 1), (what, "full preparations fed from device memory", grown, "frames behind a vertex write", want)
            assert len(probe.seen) == len(program)
            came_down = downloads_nobody_asked_for(program, probe.seen, probe.stale)
            assert not came_down, (what, "V, NB or the indices came down behind an op that has no download of its own", came_down)


@pytest.mark.parametrize("seed", range(8))
def test_dynamic_programs_under_device_fed_preparations(gpu_ctx, seed):
    """The dynamic profile's programs (the mixed world: move_spheres, three meshes, both heaps built on the device) with refit 0 and
    prepare_device 1: against the model and against the default run."""
    program = cs.make_program(seed, profile="dynamic")
    model = cs.run_model(program, profile="dynamic")
    plain = run(gpu_ctx, program, UNDEFERRED, profile="dynamic")
    check(f"seed {seed}: the default run against the model", program, plain, model)
    for cfg in (UNDEFERRED, (0, 2)):
        prepared = gpu_ctx.prepare_stats()["device"]
        got = run(gpu_ctx, program, cfg, dict(refit=0, prepare_device=1), profile="dynamic")
        check(f"seed {seed}, configuration {cfg}, device-fed, against the model", program, got, model)
        check(f"seed {seed}, configuration {cfg}, device-fed, against the default run", program, got, plain)
        assert got[2]["rays"] == plain[2]["rays"] and got[2]["watchdog_trips"] == 0, (seed, cfg)
        assert gpu_ctx.prepare_stats()["device"] > prepared, (seed, cfg, "no preparation was fed from device memory")


def test_the_replay_notices_a_missing_op(gpu_ctx):
    """The comparison is not vacuous on the GPU side: the run of a program differs from the model of that program with one op left out
    (the first of its kind) — motion_blur and the kinds the solo world gives another meaning or another kernel path."""
    noticed = set()
    kinds = ("motion_blur", "camera", "morph", "device_heap", "skin", "set_device", "set_host", "deform", "move_mesh", "bind_result")
    for seed in range(6):
        program = cs.make_program(seed, profile="solo")
        plain = run(gpu_ctx, program, UNDEFERRED, TABLE_ON)
        for kind in kinds:
            at = [i for i, op in enumerate(program) if op[0] == kind]
            if at and kind not in noticed:
                other = cs.run_model([op for i, op in enumerate(program) if i != at[0]], profile="solo")
                renumbered = ([(i - (i > at[0]), k, a) for i, k, a in plain[0]], plain[1])
                if cs.first_difference(renumbered, other) is not None:
                    noticed.add(kind)
    print("solo kinds whose removal the replay noticed:", sorted(noticed))
    assert noticed == set(kinds), (set(kinds) - noticed, "left out without the replay noticing")


# ---- directed protocols --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    """The sequential model of each protocol, made once."""
    return {}


def model_of(models, name, ops, **shape):
    if name not in models:
        models[name] = cs.run_model(ops, profile="solo", threads=16, **shape)
    return models[name]


def submissions(*parts):
    """One-frame submissions as test_gpu_command_stream.protocol makes them (frame into X0, pipelined readback, two tickets in flight): an
    int is that many of them, a list is ops played between two of them -> (ops, [index of each frame's read_begin])."""
    ops, marks, tickets = [], [], 0
    for part in parts:
        if not isinstance(part, int):
            ops += part
            continue
        for _ in range(part):
            ops.append(("frame", "X0"))
            if tickets == 2:
                ops.append(("read_end",))
                tickets -= 1
            ops.append(("read_begin", "X0", "RGBA32F"))
            marks.append(len(ops) - 1)
            tickets += 1
    return ops + [("read_end",)] * tickets, marks


def frames_of(run_or_model):
    return [a for _, k, a in run_or_model[0] if k == "read_end"]


def tile_mask(listed, height, width):
    """(tiles_y, tiles_x) bools -> (height, width): each tile's value over its 8 x 8 pixels (row 0 is the bottom in both)."""
    return np.repeat(np.repeat(listed, 8, axis=0), 8, axis=1)[:height, :width]


@pytest.fixture(scope="module")
def still(gpu_ctx, models):
    """Six one-frame submissions with nothing between them, overlapped, the table forced -> (the model, the run, its table)."""
    ops, _ = submissions(6)
    want = model_of(models, "still", ops, **SHAPE)
    got = run(gpu_ctx, ops, (0, 2), TABLE_ON, **SHAPE)
    check("still: overlapped against the model", ops, got, want)
    table = gpu_ctx.read_tile_entry()[0]
    assert table.shape == (15, 25, 8) and (table[..., 0] == DONE).any() and (table[..., 0] != DONE).any()
    # the table's rows are the image's (row 0 at the bottom): every pixel whose camera ray hits the mesh lies in a listed tile
    guide = cs.run_model([("aov", "G", 15, False)], profile="solo", threads=16, **SHAPE)[1]["Gn"]
    mesh = guide[..., 3] == 3.0
    listed = tile_mask(table[..., 0] != DONE, SHAPE["height"], SHAPE["width"])
    print(f"still: {int(mesh.sum())} mesh pixels, {int((mesh & ~listed).sum())} outside the listed tiles ({int((mesh & ~listed[::-1]).sum())} with the rows flipped)")
    assert mesh.sum() > 100 and not (mesh & ~listed).any(), "tile_mask does not read the table as the image lies"
    return want, got, table


def edited_run(gpu_ctx, models, name, parts, options, cfg=(0, 2)):
    """submissions(*parts) under cfg with `options` -> (ops, marks, model, run, launch infos per frame, table after it, tables built);
    the run equals the model and the undeferred run without the table."""
    ops, marks = submissions(*parts)
    want = model_of(models, name, ops, **SHAPE)
    if name + " plain" not in models:
        models[name + " plain"] = run(gpu_ctx, ops, UNDEFERRED, TABLE_OFF, **SHAPE)
    plain = models[name + " plain"]
    check(f"{name}: undeferred, without the table, against the model", ops, plain, want)
    before = gpu_ctx.read_tile_entry()[1]
    got = run(gpu_ctx, ops, cfg, options, **SHAPE)
    table, builds = gpu_ctx.read_tile_entry()
    check(f"{name}: {cfg} with {options} against the model", ops, got, want)
    check(f"{name}: {cfg} with {options} against undeferred", ops, got, plain)
    assert got[2]["watchdog_trips"] == 0 and plain[2]["watchdog_trips"] == 0 and got[2]["rays"] == plain[2]["rays"], name
    ls = launches(got[3], ops)
    assert len(ls) == len(marks) and all(i["n_frames"] == 1 and i["trace_stream"] in (1, 2) for i in ls), ls
    assert ls[1]["overlapped"] == 1, "the undisturbed second launch does not overlap: the protocol shows nothing"
    return ops, marks, want, got, ls, table, builds - before


@pytest.mark.parametrize("tile_entry", [-1, 1])
def test_a_camera_change_between_submissions_on_alternating_trace_streams(gpu_ctx, models, still, tile_entry):
    """1.  The launch behind the change needs another table while the launch in front of it may still read the old one, on the other
    trace stream.  Frames before the change are the old camera's, frames after it the new one's."""
    _, _, want, got, ls, table, built = edited_run(gpu_ctx, models, "camera change", (3, [("camera", 1)], 3), dict(tile_entry=tile_entry))
    base = frames_of(still[0])
    mine = frames_of(want)
    assert all(cs.same(a, b) for a, b in zip(mine[:3], base[:3])) and not any(cs.same(a, b) for a, b in zip(mine[3:], base[3:])), \
        "the camera change does not show in the model's frames: the protocol proves nothing"
    assert table.shape == still[2].shape and (table != still[2]).any(axis=2).any(), "the table behind the change is the old camera's"
    assert built == 2, ("tables built", built)
    used = [i["tile_entry"] for i in ls]
    print(f"tile_entry {tile_entry}: launches used the table {used}; the launch behind the change: overlapped = {ls[3]['overlapped']}, "
          f"trace_stream = {ls[3]['trace_stream']}; streams {[i['trace_stream'] for i in ls]}")
    assert used == ([0, 1, 1, 0, 1, 1] if tile_entry < 0 else [1] * 6), used       # auto: not for the first launch of a camera
    assert {ls[2]["trace_stream"], ls[3]["trace_stream"]} == {1, 2}, "the launches around the change share a stream: nothing is crossed"


def test_the_blob_grows_and_shrinks_between_submissions(gpu_ctx, models, still):
    """2.  deform 1.25, then deform 0.75: the frames change in tiles the old table lists as empty.  Measured with both epochs taken out of
    the table's key (a scratch build): this protocol then fails by its count of tables built, NOT by its pixels — the changed pixels in
    old-empty tiles are mostly the blob's indirect light on the ground, which the table does not touch, and the grown blob's own
    camera-ray hits stay within a tile of the old ones; protocol 3 fails in its pixels under that mutation."""
    parts = (2, [("deform", 1.25)], 2, [("deform", 0.75)], 2)
    _, _, want, got, ls, table, built = edited_run(gpu_ctx, models, "deform", parts, TABLE_ON)
    base, mine = frames_of(still[0]), frames_of(want)
    h, w = SHAPE["height"], SHAPE["width"]
    empty = tile_mask(still[2][..., 0] == DONE, h, w)
    changed = (mine[2].view(np.uint32) != base[2].view(np.uint32)).any(axis=-1)
    print(f"deform 1.25 changes {int(changed.sum())} pixels of frame 2, {int((changed & empty).sum())} of them in tiles the old table lists as empty")
    assert (changed & empty).any(), "the grown blob stays inside the tiles the old table lists: a stale table would show nothing"
    assert cs.same(mine[1], base[1]) and not cs.same(mine[4], base[4]) and not cs.same(mine[4], mine[2])
    assert built == 3 and [i["tile_entry"] for i in ls] == [1] * 6, (built, ls)      # the still blob's, the grown one's, the shrunk one's
    assert table.shape == still[2].shape and (table != still[2]).any(), "the last table is the still blob's: 1.25 x 0.75 is not 1"


def test_device_writes_and_device_heaps_between_submissions_device_fed(gpu_ctx, models, still):
    """3.  skin, morph and SetDataDevice, each with the heap built on the device, under refit 0 and prepare_device 1: the full preparation,
    the cone words and the table's rebuild all follow an un-waited device write while the previous launch may still run."""
    edits = [("device_heap", ("skin", 2, True, LO, NV)), ("device_heap", ("morph", 1, True, False)), ("device_heap", ("set_device", LO, NV, 1.25))]
    parts = (2, [edits[0]], 2, [edits[1]], 2, [edits[2]], 2)
    prepared = gpu_ctx.prepare_stats()
    _, _, want, got, ls, table, built = edited_run(gpu_ctx, models, "device writes", parts, DEVICE_FED)
    after = gpu_ctx.prepare_stats()
    mine, base = frames_of(want), frames_of(still[0])
    assert cs.same(mine[1], base[1]) and not cs.same(mine[2], base[2]), "the skin does not show: the protocol proves nothing"
    for k, n in ((1, 4), (2, 6)):                                # each later edit against the model of the protocol without it
        rest = [p for j, p in enumerate(parts) if j != 2 * k + 1]
        without = frames_of(model_of(models, f"device writes without edit {k}", submissions(*rest)[0], **SHAPE))
        assert cs.same(mine[n - 1], without[n - 1]) and not cs.same(mine[n], without[n]), (k, "the edit does not show: the protocol proves nothing")
    assert after["device"] - prepared["device"] >= 3 and built == 4, (prepared, after, built)
    assert [i["tile_entry"] for i in ls] == [1] * 8, ls


@pytest.mark.parametrize("order", ["small first", "large first"])
def test_the_table_allocation_grows_and_is_reused_across_runs(gpu_ctx, models, order):
    """4.  A 16 x 8 run and the 200 x 120 run on one fresh context, in both orders, one-frame launches on the trace streams with the table
    forced: the second run's table is another allocation (grown) or a part of the first one's.  The two runs are separated by the
    synchronisation at the end of a run, so no launch still reads the old table when it grows: this holds the growth and the reuse of
    the allocation and the pixels behind them, NOT the wait for an in-flight reader (hipEventSynchronize of te_used[] in
    tile_entry_for_launch)."""
    from unityraytracer_amd import Context
    ops, _ = submissions(4)
    small = dict(width=16, height=8, bounces=2)
    shapes = [small, SHAPE] if order == "small first" else [SHAPE, small]
    with Context(gpu_ctx.device) as own:
        tables = []
        for n, shape in enumerate(shapes):
            want = model_of(models, f"grow {shape['width']}", ops, **shape)
            got = run(own, ops, (1, 2), TABLE_ON, **shape)
            check(f"the table grows, {order}, run {n} against the model", ops, got, want)
            assert got[2]["watchdog_trips"] == 0 and 1 in used_the_table(got, ops)
            tables.append(own.read_tile_entry())
    (a, builds_a), (b, builds_b) = tables
    assert a.shape != b.shape and {a.shape, b.shape} == {(1, 2, 8), (15, 25, 8)} and builds_b > builds_a >= 1, (a.shape, b.shape, builds_a, builds_b)
    assert (a[..., 0] != DONE).any() and (b[..., 0] != DONE).any(), "a table lists nothing: the protocol proves nothing"


def test_bind_result_between_submissions_hits_the_cache(gpu_ctx, models, still):
    """5.  The other Result texture under the same camera: the table is the same one, on whichever trace stream the launch lands."""
    _, _, want, got, ls, table, built = edited_run(gpu_ctx, models, "bind_result", (3, [("bind_result",)], 3), TABLE_ON)
    assert built == 1 and [i["tile_entry"] for i in ls] == [1] * 6, (built, ls)
    assert np.array_equal(table, still[2])
    assert want[1]["T0"].any() and want[1]["T1"].any() and not cs.same(want[1]["T0"], want[1]["T1"]), "one Result texture was never written"
    assert all(cs.same(a, b) for a, b in zip(frames_of(want), frames_of(still[0]))), "the swap changes the presented frames"
    print("launch behind bind_result: overlapped =", ls[3]["overlapped"], " trace_stream =", ls[3]["trace_stream"])


BLUR_PRE = [("frame", None), ("history", 0.0), ("aov", "P", 11, False), ("camera", 1), ("aov", "G", 15, False), ("reproject", "plain", 0, 8.0, "C")]


def overlapped_run(gpu_ctx, models, name, bind):
    """BLUR_PRE + protocol(bind), as tests/test_gpu_command_stream_dynamic.py's overlapped_run -> launch_info() of the launch behind `bind`."""
    ops, mark = protocol(bind)
    ops, mark = BLUR_PRE + ops, mark + len(BLUR_PRE)
    want = model_of(models, name, ops, **SHAPE)
    stats = []
    cs.run_model(BLUR_PRE + [("frame", None), bind[0]], profile="solo", threads=16, stats=stats, **SHAPE)
    blur = [f for _, k, f in stats if k == "motion_blur"]
    assert blur and blur[0]["changed"] > 0, "the blur changes nothing: the protocol proves nothing"
    plain = run(gpu_ctx, ops, UNDEFERRED, TABLE_OFF, **SHAPE)
    got = run(gpu_ctx, ops, (0, 2), TABLE_ON, **SHAPE)
    check(f"{name}: undeferred against the model", ops, plain, want)
    check(f"{name}: overlapped against undeferred", ops, got, plain)
    assert got[2]["watchdog_trips"] == 0 and plain[2]["watchdog_trips"] == 0
    ls = launches(got[3], ops)
    assert all(i["n_frames"] == 1 and i["trace_stream"] in (1, 2) for i in ls), ls
    assert ls[1]["overlapped"] == 1, "the undisturbed second launch does not overlap: the protocol shows nothing"
    return dict(got[3])[mark]


def test_motion_blur_writes_the_bound_result_between_two_submissions(gpu_ctx, models):
    """6a.  motion_blur writes the Result texture on the main stream, and the launch that follows writes the same texture: it waits."""
    marked = overlapped_run(gpu_ctx, models, "blur into the bound Result", [("motion_blur", "C", "Gh", "T0", 1)])
    assert marked["overlapped"] == 0, "the launch into the texture motion blur has just written does not wait for it"


def test_motion_blur_writes_what_is_bound_as_the_sky_and_traced_at_once(gpu_ctx, models):
    """6b."""
    marked = overlapped_run(gpu_ctx, models, "blur into the next sky", [("motion_blur", "C", "Gh", "X1", 1), ("bind_sky", "X1")])
    assert marked["overlapped"] == 0, "the launch that samples what motion blur has just written does not wait for it"


def test_the_motion_blur_scratch_grows_between_deferred_frames(gpu_ctx, models):
    """7.  tests/test_gpu_command_stream_dynamic.py's protocol 7 with motion_blur in place of dof.  urt_motion_blur takes four textures of
    ONE size, so the low grid of the display world cannot feed it: the test makes a second set of frame textures at the low size (75 x 48:
    colour, motion and hit set from the model of the same world at that size, two destinations) on a context that has run nothing, and
    plays them from the probe, between the ops of ONE run with nothing waited for: frame, LOW blur, frame, the 200 x 120 blur — it
    needs more scratch than the context has made, while the low blur and a frame are still in flight —, frame, LOW blur of what the
    first one wrote, frame.  The frame-sized textures equal the model of the program (the probe's blurs touch none of them), the low
    destinations equal tests/motion_blur_ref.py on the low inputs."""
    import motion_blur_ref
    from unityraytracer_amd import Context, RenderTexture
    w, h = SHAPE["width"], SHAPE["height"]
    lw, lh = cs.low_size(w, h)
    assert lw * lh < w * h
    low = cs.run_model(BLUR_PRE, profile="solo", threads=16, **dict(SHAPE, width=lw, height=lh))[1]
    first = motion_blur_ref.motion_blur_ref(low["C"], low["MV"], low["Gh"], **cs.MBLUR[1])
    second = motion_blur_ref.motion_blur_ref(first, low["MV"], low["Gh"], **cs.MBLUR[0])
    assert first.shape == (lh, lw, 4) and not cs.same(first, low["C"]) and not cs.same(second, first), "a low blur changes nothing: the protocol proves nothing"
    ops = BLUR_PRE + [("frame", None), ("frame", None), ("motion_blur", "C", "Gh", "X0", 0), ("frame", None), ("frame", None)]
    at = len(BLUR_PRE)
    stats = []
    want = cs.run_model(ops, profile="solo", threads=16, stats=stats, **SHAPE)
    assert [f["changed"] > 0 for _, k, f in stats if k == "motion_blur"] == [True], "the full-size blur changes nothing: the protocol proves nothing"
    for cfg in (UNDEFERRED,) + DEFERRING:
        with Context(gpu_ctx.device) as own:
            tex = {n: RenderTexture(own, lw, lh) for n in ("src", "motion", "hit", "dst1", "dst2")}
            try:
                for n, a in (("src", low["C"]), ("motion", low["MV"]), ("hit", low["Gh"])):
                    tex[n].SetPixels(a)
                played = []

                def low_blurs(i, op, m, pw):                     # (ops of its own between the program's: they submit what is deferred, as any blur does)
                    if i == at:
                        own.motion_blur(tex["src"], tex["motion"], tex["hit"], tex["dst1"], **cs.MBLUR[1])
                        played.append(i)
                    elif i == at + 3:
                        own.motion_blur(tex["dst1"], tex["motion"], tex["hit"], tex["dst2"], **cs.MBLUR[0])
                        played.append(i)

                got = run(own, ops, cfg, TABLE_ON, probe=low_blurs, **SHAPE)
                check(f"blur scratch growth, configuration {cfg} against the model", ops, got, want)
                assert got[2]["watchdog_trips"] == 0 and played == [at, at + 3], (cfg, played)
                assert cs.same(tex["dst1"].GetPixels(), first), (cfg, "the low blur in front of the growth")
                assert cs.same(tex["dst2"].GetPixels(), second), (cfg, "the low blur behind the growth")
            finally:
                for t in tex.values():
                    t.Release()
