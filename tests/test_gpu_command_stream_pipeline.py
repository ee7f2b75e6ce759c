"""GPU: program order for the image-space and device-side calls around the frame loop (the "pipeline" profile of
tests/command_stream.py): feature buffers, reprojection in its three forms, the denoiser, pixel selection and resampling, pixel-mode and
device-form queries, and the two-sided vertex and normal buffers (skinning, normals, device and host SetData, snapshots, readbacks).

Fuzz: with nothing deferred (frames_per_launch 1, overlap_launches 0) a random program equals the sequential model — observations, the
final contents of every texture and both sides of every buffer — bit for bit (the denoised image within the bound include/urt.h states,
see command_stream.same); every deferring configuration equals that run bit for bit, the ray counter included.  The reach of the seed
set is held by tests/test_command_stream_model.py.

Directed protocols: where the library exposes its bookkeeping the protocol asserts on that — downloads, in-place preparations, the
overlap of a launch — once per configuration; none reruns to catch a race by luck."""
import pytest

import command_stream as cs
from test_gpu_command_stream import DEFERRING, SHAPE, UNDEFERRED, launches, protocol

pytestmark = pytest.mark.gpu

CONFIGS = (UNDEFERRED,) + DEFERRING


def check(what, program, got, want):
    d = cs.first_difference(got, want, radiance=True)
    if d is not None:
        upto, text = d
        raise AssertionError(f"{what}: {text}\nops{'' if upto is None else ' up to it'}:\n{cs.describe(program, upto)}")


def run(gpu_ctx, program, cfg, **kw):
    return cs.run_gpu(gpu_ctx, program, *cfg, profile="pipeline", **kw)


@pytest.mark.parametrize("seed", range(24))
def test_random_pipeline_programs_keep_program_order(gpu_ctx, seed):
    program = cs.make_program(seed, profile="pipeline")
    model = cs.run_model(program, profile="pipeline")
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
    """The comparison is not vacuous on the GPU side either: the run of a program differs from the model of that program with one
    writing op left out."""
    noticed = set()
    for seed in range(4):
        program = cs.make_program(seed, profile="pipeline")
        plain = run(gpu_ctx, program, UNDEFERRED)
        for kind in ("aov_into", "reproject", "skin", "set_device", "set_host", "normals"):
            at = [i for i, op in enumerate(program) if op[0] == kind]
            if at and kind not in noticed:
                other = cs.run_model([op for i, op in enumerate(program) if i != at[0]], profile="pipeline")
                renumbered = ([(i - (i > at[0]), k, a) for i, k, a in plain[0]], plain[1])
                if cs.first_difference(renumbered, other) is not None:
                    noticed.add(kind)
    assert len(noticed) >= 5, noticed


# ---- directed protocols --------------------------------------------------------------------------------------------------------------
LO, HI = cs.pipeline_world()["span"]
NV = len(cs.pipeline_world()["rest_v"])


@pytest.fixture(scope="module")
def models():
    """The sequential model of each protocol, made once."""
    return {}


def run_all(gpu_ctx, models, name, ops, probe=None, **shape):
    """The protocol under every configuration, each once -> [(configuration, run)]; the undeferred run equals the model, the others equal it."""
    if name not in models:
        models[name] = cs.run_model(ops, profile="pipeline", threads=16, **shape)
    runs = []
    for cfg in CONFIGS:
        if probe is not None:
            probe.seen = []
        got = run(gpu_ctx, ops, cfg, probe=probe, **shape)
        check(f"{name}, configuration {cfg} against the model", ops, got, models[name])
        assert got[2]["watchdog_trips"] == 0, (name, cfg)
        runs.append((cfg, got, list(probe.seen) if probe is not None else None))
    for cfg, got, _ in runs[1:]:
        check(f"{name}, configuration {cfg} against {UNDEFERRED}", ops, got, runs[0][1])
        assert got[2]["rays"] == runs[0][1][2]["rays"], (name, cfg)
    return runs


def bookkeeping(gpu_ctx):
    """A probe that records, after every op, what the library says of the vertex buffer and of its scene preparations (none of these
    calls submits or waits)."""
    def probe(i, op, m, pw):
        probe.seen.append((i, gpu_ctx.buffer_state(pw.V), gpu_ctx.refit_stats(), gpu_ctx.deform_stats()))
    probe.seen = []
    return probe


def test_skin_then_frame_refits_without_a_download(gpu_ctx, models):
    ops = [("frame", None), ("get", "T0"), ("skin", 0, True, LO, HI - LO + 1), ("frame", None), ("get", "T0")]
    for cfg, got, seen in run_all(gpu_ctx, models, "skin then frame", ops, bookkeeping(gpu_ctx)):
        before, after = seen[1], seen[4]                          # after the first readback (all submitted), after the last
        assert after[1]["downloads"] == before[1]["downloads"], (cfg, "the skinned positions were downloaded")
        assert after[1]["mirror_bytes"] == NV * 12 and seen[2][1]["stale_first"] == LO and seen[2][1]["stale_last"] == HI, (cfg, seen[2][1])
        assert after[2][1] == before[2][1] + 1, (cfg, "the skinned scene was not prepared in place", before[2], after[2])
        assert after[3]["deformed"] == before[3]["deformed"] + 1 and after[3]["forced_rebuilds"] == before[3]["forced_rebuilds"], (cfg, after[3])
        assert not cs.same(got[0][0][2], got[0][1][2]), "the pose does not show in the frame: the protocol proves nothing"


def test_set_host_then_get_buffer_downloads_nothing(gpu_ctx, models):
    ops = [("frame", None), ("set_host", LO + 5, 20, 0.9), ("get_buffer", "V", LO, 40), ("frame", None), ("get", "T0")]
    for cfg, got, seen in run_all(gpu_ctx, models, "set_host then get_buffer", ops, bookkeeping(gpu_ctx)):
        assert seen[0][1]["mirror_bytes"] == NV * 12, "the vertex buffer has no mirror: the protocol proves nothing"
        assert seen[2][1]["downloads"] == seen[0][1]["downloads"], (cfg, seen[0][1], seen[2][1])
        assert seen[2][1]["stale_first"] > seen[2][1]["stale_last"], (cfg, seen[2][1])


def test_async_query_answers_for_the_scene_at_its_call(gpu_ctx, models):
    ops = [("frame", None), ("ray_query_async", 5), ("radiance_async", 5), ("deform", 0.75), ("frame", None), ("get", "T0")]
    runs = run_all(gpu_ctx, models, "async query, then an edit", ops)
    # (the model's own answers: the edit changes them, so an answer for the edited scene would not pass)
    late = cs.run_model(ops[:1] + ops[3:4] + ops[1:3] + ops[4:], profile="pipeline")
    early = models["async query, then an edit"]
    for n in (0, 1):
        assert early[0][n][1] == late[0][n][1] == ("ray_query_async", "radiance_async")[n]
        assert not cs.same(early[0][n][2], late[0][n][2]), "the edit does not change the query's answer: the protocol proves nothing"
    assert len(runs) == len(CONFIGS)


def test_eight_host_uploads_in_a_row_then_a_frame(gpu_ctx, models):
    """More ranged SetData calls into the mirrored vertex buffer than the ring of pinned upload slots holds, with nothing waited for in between."""
    uploads = [("set_host", LO + 11 * n, 9 + n, (0.9, 1.25, 0.75)[n % 3]) for n in range(8)]
    ops = [("frame", None)] + uploads + [("frame", None), ("get", "T0"), ("get_buffer", "V", 0, NV), ("bounds", 0, NV)]
    runs = run_all(gpu_ctx, models, "eight uploads", ops, bookkeeping(gpu_ctx))
    for cfg, got, seen in runs:
        assert seen[-1][1]["downloads"] == seen[0][1]["downloads"], (cfg, "a host upload was downloaded again")


def test_aov_into_the_bound_result_between_two_submissions(gpu_ctx, models):
    """One-frame submissions on alternating trace streams (overlap_launches 2); between two of them render_aov writes the Result texture on
    the main stream.  The launch that follows writes the same texture: it must wait for the feature-buffer kernel (launch_info: not
    overlapped), and every frame equals the model.  Control: feature buffers into G alone leave every frame as it is without them."""
    ops, mark = protocol([("aov_into", "T0")])
    if "aov_into" not in models:
        models["aov_into"] = cs.run_model(ops, profile="pipeline", threads=16, **SHAPE)
    plain = run(gpu_ctx, ops, UNDEFERRED, **SHAPE)
    got = run(gpu_ctx, ops, (0, 2), **SHAPE)
    check("aov_into: undeferred against the model", ops, plain, models["aov_into"])
    check("aov_into: overlapped against undeferred", ops, got, plain)
    ls = launches(got[3], ops)
    assert all(i["n_frames"] == 1 and i["trace_stream"] in (1, 2) for i in ls), ls
    assert ls[1]["overlapped"] == 1, "the undisturbed second launch does not overlap: the protocol shows nothing"
    assert dict(got[3])[mark]["overlapped"] == 0, "the launch into the texture render_aov has just written does not wait for it"
    assert got[2]["watchdog_trips"] == 0 and plain[2]["watchdog_trips"] == 0
    # control
    with_g, _ = protocol([("aov", "G", 15, False)])
    without, _ = protocol([])
    a = run(gpu_ctx, with_g, (0, 2), **SHAPE)
    b = run(gpu_ctx, without, (0, 2), **SHAPE)
    assert len(a[0]) == len(b[0]) and all(cs.same(x[2], y[2]) for x, y in zip(a[0], b[0])), "feature buffers into G changed a frame"
    assert all(cs.same(a[1][n], b[1][n]) for n in cs.FRAME_TEX), "feature buffers into G changed a frame texture"
    assert a[1]["Gh"].any() and not b[1]["Gh"].any()
    assert a[2]["rays"] == b[2]["rays"]
