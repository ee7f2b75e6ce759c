"""GPU: program order for blend shapes, the object-level heaps built on the device and depth of field (the "dynamic" profile of
tests/command_stream.py): urt_morph_vertices under a weight table the host rewrites between calls, urt_mesh_leaf_bounds_device /
urt_sphere_leaf_bounds_device / urt_build_object_bvh_device into the very heap buffer bound to the scene — between deferred frames,
behind host uploads through the ring, morphs, skins and un-waited queries, read back and overwritten by the host — and
urt_depth_of_field with its grow-only scratch, on its own and inside RayTraceMaster.ToneMap.

Fuzz: with nothing deferred (frames_per_launch 1, overlap_launches 0) a random program equals the sequential model bit for bit —
observations, every texture of every size class, both sides of V NB SNAP W LM LS HM HS, the exposure states, the master's tone-mapped
texture and its hit guide; only the denoised image is held to urt_denoise's bound.  Every deferring configuration equals that run bit
for bit, the ray counter included.  The reach of the seed set is held by tests/test_command_stream_model.py.

Directed protocols: each runs once per configuration and none reruns; each asserts that it shows something."""
import pytest

import command_stream as cs
from test_gpu_command_stream import DEFERRING, SHAPE, UNDEFERRED, launches, protocol

pytestmark = pytest.mark.gpu

CONFIGS = (UNDEFERRED,) + DEFERRING
LO, HI = cs.dynamic_world()["span"]
NV = len(cs.dynamic_world()["rest_v"])
COUNTS = cs.dynamic_world()["counts"]


def check(what, program, got, want):
    d = cs.first_difference(got, want, radiance=True)
    if d is not None:
        upto, text = d
        raise AssertionError(f"{what}: {text}\nops{'' if upto is None else ' up to it'}:\n{cs.describe(program, upto)}")


def run(ctx, program, cfg, **kw):
    return cs.run_gpu(ctx, program, *cfg, profile="dynamic", **kw)


@pytest.mark.parametrize("seed", range(24))
def test_random_dynamic_programs_keep_program_order(gpu_ctx, seed):
    program = cs.make_program(seed, profile="dynamic")
    model = cs.run_model(program, profile="dynamic")
    assert all(n in model[1] and n + ".dev" in model[1] for n in cs.DYN_BUFFERS)
    plain = run(gpu_ctx, program, UNDEFERRED)
    check(f"seed {seed}, configuration {UNDEFERRED} against the model", program, plain, model)
    assert plain[2]["watchdog_trips"] == 0
    for cfg in DEFERRING:
        got = run(gpu_ctx, program, cfg)
        check(f"seed {seed}, configuration {cfg} against {UNDEFERRED}", program, got, plain)
        assert got[2]["rays"] == plain[2]["rays"], (seed, cfg, got[2]["rays"], plain[2]["rays"])
        assert got[2]["dispatches"] == plain[2]["dispatches"] and got[2]["launches"] <= plain[2]["launches"], (seed, cfg)
        assert got[2]["watchdog_trips"] == 0, (seed, cfg)


def test_the_replay_notices_a_missing_op(gpu_ctx):
    """The comparison is not vacuous on the GPU side: the run of a program differs from the model of that program with one op of a
    dynamic kind left out (the first of its kind)."""
    noticed = set()
    for seed in range(4):
        program = cs.make_program(seed, profile="dynamic")
        plain = run(gpu_ctx, program, UNDEFERRED)
        for kind in ("morph", "dof", "device_heap", "rebuild_heap", "master_dof"):
            at = [i for i, op in enumerate(program) if op[0] == kind]
            if at and kind not in noticed:
                other = cs.run_model([op for i, op in enumerate(program) if i != at[0]], profile="dynamic")
                renumbered = ([(i - (i > at[0]), k, a) for i, k, a in plain[0]], plain[1])
                if cs.first_difference(renumbered, other) is not None:
                    noticed.add(kind)
    assert len(noticed) >= 4, noticed


# ---- directed protocols --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    """The sequential model of each protocol, made once."""
    return {}


def model_of(models, name, ops, **shape):
    if name not in models:
        models[name] = cs.run_model(ops, profile="dynamic", threads=16, **shape)
    return models[name]


def run_all(ctx, models, name, ops, probe=None, fresh_context=False, **shape):
    """The protocol under every configuration, each once -> [(configuration, run, what the probe saw)]; the undeferred run equals the
    model, the others equal it.  fresh_context: each run on a context of its own (its scratch starts empty)."""
    from unityraytracer_amd import Context
    want = model_of(models, name, ops, **shape)
    runs = []
    for cfg in CONFIGS:
        if probe is not None:
            probe.seen = []
        if fresh_context:
            with Context(ctx.device) as own:
                got = run(own, ops, cfg, probe=probe, **shape)
        else:
            got = run(ctx, ops, cfg, probe=probe, **shape)
        check(f"{name}, configuration {cfg} against the model", ops, got, want)
        assert got[2]["watchdog_trips"] == 0, (name, cfg)
        runs.append((cfg, got, list(probe.seen) if probe is not None else None))
    for cfg, got, _ in runs[1:]:
        check(f"{name}, configuration {cfg} against {UNDEFERRED}", ops, got, runs[0][1])
        assert got[2]["rays"] == runs[0][1][2]["rays"], (name, cfg)
    return runs


def bookkeeping(gpu_ctx):
    """A probe that records, after every op, what the library says of the vertex buffer, of the bound mesh heap and of its scene
    preparations (none of these calls submits or waits)."""
    def probe(i, op, m, pw):
        probe.seen.append((i, gpu_ctx.buffer_state(pw.V), gpu_ctx.refit_stats(), gpu_ctx.deform_stats(), gpu_ctx.buffer_state(pw.HM)))
    probe.seen = []
    return probe


def test_morph_then_a_device_heap_then_a_frame(gpu_ctx, models):
    """1.  The pose shows in the second frame; the morphed positions never cross the bus, the scene is prepared in place, and the heap
    costs the ONE synchronising download every device-written small table gets at the next preparation (DESIGN.md section 29;
    tests/test_gpu_object_bvh_master.py: MorphMeshes downloads {"vertices": 0, "normals": 0, "mesh_bvh": 1, "sphere_bvh": 0})."""
    ops = [("frame", None), ("get", "T0"), ("device_heap", ("morph", 1, True, False)), ("frame", None), ("get", "T0")]
    for cfg, got, seen in run_all(gpu_ctx, models, "morph, device heap, frame", ops, bookkeeping(gpu_ctx)):
        before, after = seen[1], seen[4]                          # after the first readback (all submitted), after the last
        assert after[1]["downloads"] == before[1]["downloads"], (cfg, "the morphed positions were downloaded")
        assert after[1]["mirror_bytes"] == NV * 12 and seen[2][1]["stale_first"] == LO and seen[2][1]["stale_last"] == HI, (cfg, seen[2][1])
        assert after[2][1] == before[2][1] + 1, (cfg, "the morphed scene was not prepared in place", before[2], after[2])
        assert after[3]["deformed"] == before[3]["deformed"] + 1 and after[3]["forced_rebuilds"] == before[3]["forced_rebuilds"], (cfg, after[3])
        assert after[4]["downloads"] == before[4]["downloads"] + 1, (cfg, "one device build costs one download of the heap", before[4], after[4])
        assert not cs.same(got[0][0][2], got[0][1][2]), "the pose does not show in the frame: the protocol proves nothing"


def test_a_device_build_between_two_submissions_on_alternating_trace_streams(gpu_ctx, models):
    """2.  One-frame submissions on alternating trace streams; between two of them a MeshObject moves and the heap is built on the
    context's stream.  The preparation that follows downloads the heap and re-prepares the scene in place while the launch of the old
    scene may still run: frames before the build are the old scene's, frames after it the new scene's — the pixel comparison is the
    check.  What launch_info() says of the launch behind the build is recorded, and held only to being a flag."""
    ops, mark = protocol([("device_heap", ("move_mesh", 0, 1))])
    want = model_of(models, "device build between submissions", ops, **SHAPE)
    plain = run(gpu_ctx, ops, UNDEFERRED, **SHAPE)
    got = run(gpu_ctx, ops, (0, 2), **SHAPE)
    check("device build between submissions: undeferred against the model", ops, plain, want)
    check("device build between submissions: overlapped against undeferred", ops, got, plain)
    assert got[2]["watchdog_trips"] == 0 and plain[2]["watchdog_trips"] == 0 and got[2]["rays"] == plain[2]["rays"]
    ls = launches(got[3], ops)
    assert all(i["n_frames"] == 1 and i["trace_stream"] in (1, 2) for i in ls), ls
    assert ls[1]["overlapped"] == 1, "the undisturbed second launch does not overlap: the protocol shows nothing"
    marked = dict(got[3])[mark]
    print("launch behind the device build: overlapped =", marked["overlapped"], " trace_stream =", marked["trace_stream"])
    assert marked["overlapped"] in (0, 1)
    frames = [a for _, k, a in want[0] if k == "read_end"]
    assert not cs.same(frames[1], frames[2]) and len(frames) == 4, "the move does not show: the protocol proves nothing"


def test_eight_host_uploads_each_with_a_device_build_then_a_frame(gpu_ctx, models):
    """3.  More ranged SetData calls into the mirrored vertex buffer than the ring of pinned upload slots holds, each followed by the
    leaf kernel that must see it, nothing waited for in between."""
    uploads = [("device_heap", ("set_host", LO + 11 * n, 9 + n, (0.9, 1.25, 0.75)[n % 3])) for n in range(8)]
    ops = [("frame", None)] + uploads + [("frame", None), ("get", "T0"), ("get_buffer", "HM", 0, COUNTS["HM"]), ("get_buffer", "LM", 0, COUNTS["LM"]),
                                         ("get_buffer", "V", 0, NV)]
    runs = run_all(gpu_ctx, models, "eight uploads with device builds", ops, bookkeeping(gpu_ctx))
    want = models["eight uploads with device builds"]
    start = cs.run_model([("rebuild_heap", 0)] + ops[-3:], profile="dynamic")     # the leaves and the heap of the untouched scene
    assert want[0][2][1] == start[0][1][1] == "get_buffer" and not cs.same(want[0][2][2], start[0][1][2]) and \
        not cs.same(want[0][1][2], start[0][0][2]), "the uploads do not move the blob's leaf: the protocol proves nothing"
    for cfg, got, seen in runs:
        assert seen[-1][1]["downloads"] == seen[0][1]["downloads"], (cfg, "a host upload was downloaded again")


def test_a_device_built_heap_read_back_and_written_back_by_the_host(gpu_ctx, models):
    """4.  device_heap(move_spheres), GetData of the heap, SetData of those very values, frame: no pixel and no counter differs from the
    run without the write-back."""
    head = [("frame", None), ("device_heap", ("move_spheres", 1)), ("get_buffer", "HS", 0, COUNTS["HS"])]
    tail = [("frame", None), ("get", "T0"), ("get", "C")]
    ops = head + tail
    assert not cs.same(model_of(models, "heap written back", ops)[1]["HS"], cs.heap_words(cs.make_scene().sphere_bvh)), "the move changes no heap"
    for cfg in CONFIGS:
        raw = []

        def write_back(i, op, m, pw):
            if i == 2:                                           # the very bytes the readback returned, through the host's SetData
                raw.append(pw.HS.GetData())
                pw.HS.SetData(raw[0])

        without = run(gpu_ctx, ops, cfg)
        with_it = run(gpu_ctx, ops, cfg, probe=write_back)
        check(f"heap written back, configuration {cfg} against the model", ops, with_it, models["heap written back"])
        check(f"heap written back, configuration {cfg} against the run without the write-back", ops, with_it, without)
        assert len(raw) == 1 and cs.same(cs.heap_words(raw[0]), models["heap written back"][1]["HS"])
        timed = ("trace_ms",)                                    # (a duration, not a count)
        assert {k: v for k, v in with_it[2].items() if k not in timed} == {k: v for k, v in without[2].items() if k not in timed}, \
            (cfg, "a counter differs", with_it[2], without[2])


def test_async_query_answers_for_the_scene_before_the_device_build(gpu_ctx, models):
    """5.  tests/test_gpu_command_stream_pipeline.py's protocol with the edit and the heap on the device side."""
    ops = [("frame", None), ("ray_query_async", 5), ("radiance_async", 5), ("device_heap", ("deform", 0.75)), ("frame", None), ("get", "T0")]
    runs = run_all(gpu_ctx, models, "async query, then a device build", ops)
    late = cs.run_model(ops[:1] + ops[3:4] + ops[1:3] + ops[4:], profile="dynamic")
    early = models["async query, then a device build"]
    for n in (0, 1):
        assert early[0][n][1] == late[0][n][1] == ("ray_query_async", "radiance_async")[n]
        assert not cs.same(early[0][n][2], late[0][n][2]), "the edit does not change the query's answer: the protocol proves nothing"
    assert len(runs) == len(CONFIGS)


DOF_PRE = [("aov", "G", 15, False)]                              # the hit image ("dof", ...) works on, in front of the protocol


def overlapped_run(gpu_ctx, models, name, bind):
    """DOF_PRE + protocol(bind), as tests/test_gpu_command_stream_display.py's overlapped_run -> launch_info() of the launch behind `bind`."""
    ops, mark = protocol(bind)
    ops, mark = DOF_PRE + ops, mark + len(DOF_PRE)
    want = model_of(models, name, ops, **SHAPE)
    plain = run(gpu_ctx, ops, UNDEFERRED, **SHAPE)
    got = run(gpu_ctx, ops, (0, 2), **SHAPE)
    check(f"{name}: undeferred against the model", ops, plain, want)
    check(f"{name}: overlapped against undeferred", ops, got, plain)
    assert got[2]["watchdog_trips"] == 0 and plain[2]["watchdog_trips"] == 0
    ls = launches(got[3], ops)
    assert all(i["n_frames"] == 1 and i["trace_stream"] in (1, 2) for i in ls), ls
    assert ls[1]["overlapped"] == 1, "the undisturbed second launch does not overlap: the protocol shows nothing"
    return dict(got[3])[mark]


def test_depth_of_field_writes_the_bound_result_between_two_submissions(gpu_ctx, models):
    """6a.  dof joins the display writers: it writes the Result texture on the main stream, and the launch that follows writes the
    same texture — it must wait for that kernel."""
    marked = overlapped_run(gpu_ctx, models, "dof into the bound Result", [("dof", "C", "Gh", "T0", 1)])
    assert marked["overlapped"] == 0, "the launch into the texture depth of field has just written does not wait for it"


def test_depth_of_field_writes_what_is_bound_as_the_sky_and_traced_at_once(gpu_ctx, models):
    """6b."""
    marked = overlapped_run(gpu_ctx, models, "dof into the next sky", [("dof", "C", "Gh", "X1", 1), ("bind_sky", "X1")])
    assert marked["overlapped"] == 0, "the launch that samples what depth of field has just written does not wait for it"


def test_the_depth_of_field_scratch_grows_between_deferred_frames(gpu_ctx, models):
    """7.  dof on the low grid, on the frame, on the low grid again, a frame deferred in front of each, on a context that has run
    nothing larger: the second call needs more scratch than the first has made."""
    w, h = SHAPE["width"], SHAPE["height"]
    lw, lh = cs.low_size(w, h)
    assert lw * lh < w * h
    ops = [("aov_low", False), ("aov", "G", 15, False), ("frame", None), ("dof", "Lc", "Lh", "Ln", 1), ("frame", None), ("dof", "C", "Gh", "X0", 2),
           ("frame", None), ("dof", "Ln", "Lh", "Lc", 0), ("frame", None)]
    want = model_of(models, "dof scratch growth", ops, **SHAPE)
    assert all(want[1][n][..., :3].any() for n in ("Ln", "X0", "Lc")) and not cs.same(want[1]["X0"], want[1]["C"])
    run_all(gpu_ctx, models, "dof scratch growth", ops, fresh_context=True, **SHAPE)


def test_the_master_presents_with_depth_of_field_and_leaves_the_camera(gpu_ctx, models):
    """8.  ToneMap with depth of field on, a frame right behind it: C is what the frames alone make it (ToneMap never modifies it, and
    the frame after it went through the host's projection again), and TM is the four explicit calls on the guide the master rendered."""
    import dof_ref
    import tonemap_ref as tm
    j = 1
    ops = [("master_dof", j)] + [("frame", None)] * 3 + [("present_tm", None, "aces"), ("frame", None), ("get", "C"), ("get", "TM"),
                                                         ("master_dof", None), ("present_tm", None, "aces")]
    frames_only = cs.run_model([("frame", None)] * 4, profile="dynamic")[1]["C"]
    by_hand = cs.run_model([("frame", None)] * 3, profile="dynamic")[1]["C"]
    for cfg, got, _ in run_all(gpu_ctx, models, "the master with depth of field", ops):
        assert cs.same(got[0][0][2], frames_only) and cs.same(got[1]["C"], frames_only), (cfg, "ToneMap or the camera it left changed C")
        # TM after the first ToneMap (read behind the next frame) is the explicit calls on the guide the master rendered: metering,
        # depth of field, (no bloom,) tone mapping, each restated
        state = tm.auto_exposure_ref(by_hand, None, cs.fresh_state(), **cs.MASTER_EXPOSURE)
        blurred = dof_ref.dof_ref(by_hand, got[1]["DH"], **cs.DOF[j])
        assert got[1]["DH"][..., 3].any() and not cs.same(blurred, by_hand), (cfg, "the blur changes nothing: the protocol proves nothing")
        assert cs.same(got[0][1][2], tm.tonemap_ref(blurred, exposure=1.0, op=tm.ACES, state_exposure=state["exposure"])), (cfg, "TM")
        assert not cs.same(got[1]["TM"], got[0][1][2]), (cfg, "DisableDepthOfField changes nothing")
