"""GPU: program order for the display calls (the "display" profile of tests/command_stream.py): guide-driven upsampling from a low grid,
auto-exposure with its caller-owned state, tone mapping and bloom — between deferred frames, in place, into the bound Result texture
and into a texture that is bound as the sky at once — and RayTraceMaster.ToneMap against the three explicit calls it stands for.

Fuzz: with nothing deferred (frames_per_launch 1, overlap_launches 0) a random program equals the sequential model bit for bit —
observations (the exposure states included: exposure and target as bits, the counters and all 256 bins as integers), the final contents
of every texture of the three size classes, both states, the master's state and its own tone-mapped texture; every deferring
configuration equals that run bit for bit, the ray counter included.  The restatements (tests/upsample_ref.py, tests/tonemap_ref.py,
tests/bloom_ref.py) are exact: no tolerance anywhere but on the denoised image.  The reach of the seed set is held by
tests/test_command_stream_model.py.

Directed protocols: each runs once per configuration; where a race is possible the library's bookkeeping decides
(launch_info()["overlapped"]), and each protocol asserts that it shows something: the overlapped neighbour launch, the control, or
readbacks that differ."""
import numpy as np
import pytest

import command_stream as cs
from test_gpu_command_stream import DEFERRING, SHAPE, UNDEFERRED, launches, protocol

pytestmark = pytest.mark.gpu

CONFIGS = (UNDEFERRED,) + DEFERRING
WIDE = cs.WIDE_FALLBACK


def check(what, program, got, want):
    d = cs.first_difference(got, want, radiance=True)
    if d is not None:
        upto, text = d
        raise AssertionError(f"{what}: {text}\nops{'' if upto is None else ' up to it'}:\n{cs.describe(program, upto)}")


def run(ctx, program, cfg, **kw):
    return cs.run_gpu(ctx, program, *cfg, profile="display", **kw)


@pytest.mark.parametrize("seed", range(24))
def test_random_display_programs_keep_program_order(gpu_ctx, seed):
    program = cs.make_program(seed, profile="display")
    model = cs.run_model(program, profile="display")
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
    display kind left out (the first of its kind)."""
    noticed = set()
    for seed in range(4):
        program = cs.make_program(seed, profile="display")
        plain = run(gpu_ctx, program, UNDEFERRED)
        for kind in ("meter", "tonemap", "bloom", "upsample", "state_reset"):
            at = [i for i, op in enumerate(program) if op[0] == kind]
            if at and kind not in noticed:
                other = cs.run_model([op for i, op in enumerate(program) if i != at[0]], profile="display")
                renumbered = ([(i - (i > at[0]), k, a) for i, k, a in plain[0]], plain[1])
                if cs.first_difference(renumbered, other) is not None:
                    noticed.add(kind)
    assert len(noticed) >= 4, noticed


# ---- directed protocols --------------------------------------------------------------------------------------------------------------
UPSAMPLE_PRE = [("aov_low", False), ("aov", "G", 15, False)]    # what ("upsample", ...) works on, in front of the protocol


def writer_into(name, dest):
    """(the ops in front of the protocol, the writer op) of one of the three display writers, with `dest` as its destination."""
    return {"tonemap": ([], ("tonemap", "C", dest, None, "aces", 1.0)), "bloom": ([], ("bloom", "C", dest, None, 3, 0)),
            "upsample": (UPSAMPLE_PRE, ("upsample", dest, None, False, WIDE))}[name]


WRITERS = ("tonemap", "bloom", "upsample")


@pytest.fixture(scope="module")
def models():
    """The sequential model of each protocol, made once."""
    return {}


def model_of(models, name, ops):
    if name not in models:
        models[name] = cs.run_model(ops, profile="display", threads=16, **SHAPE)
    return models[name]


def run_all(ctx, models, name, ops):
    """The protocol under every configuration, each once -> [(configuration, run)]; the undeferred run equals the model, the others equal it."""
    want = model_of(models, name, ops)
    runs = []
    for cfg in CONFIGS:
        got = run(ctx, ops, cfg, **SHAPE)
        check(f"{name}, configuration {cfg} against the model", ops, got, want)
        assert got[2]["watchdog_trips"] == 0, (name, cfg)
        runs.append((cfg, got))
    for cfg, got in runs[1:]:
        check(f"{name}, configuration {cfg} against {UNDEFERRED}", ops, got, runs[0][1])
        assert got[2]["rays"] == runs[0][1][2]["rays"], (name, cfg)
    return runs


def overlapped_run(gpu_ctx, models, name, pre, bind, **kw):
    """pre + protocol(bind) with nothing deferred (equals the model) and as one-frame submissions on alternating trace streams (equals
    that run) -> (the overlapped run, the launches after each readback's submission, launch_info() of the launch that follows `bind`)."""
    ops, mark = protocol(bind, **kw)
    ops, mark = pre + ops, mark + len(pre)
    want = model_of(models, name, ops)
    plain = run(gpu_ctx, ops, UNDEFERRED, **SHAPE)
    got = run(gpu_ctx, ops, (0, 2), **SHAPE)
    check(f"{name}: undeferred against the model", ops, plain, want)
    check(f"{name}: overlapped against undeferred", ops, got, plain)
    assert got[2]["watchdog_trips"] == 0 and plain[2]["watchdog_trips"] == 0
    ls = launches(got[3], ops)
    assert all(i["n_frames"] == 1 and i["trace_stream"] in (1, 2) for i in ls), ls          # one-frame submissions on the trace streams
    assert ls[1]["overlapped"] == 1, "the undisturbed second launch does not overlap: the protocol shows nothing"
    return got, ls, dict(got[3])[mark]


@pytest.mark.parametrize("writer", WRITERS)
def test_a_display_call_writes_the_bound_result_between_two_submissions(gpu_ctx, models, writer):
    """One-frame submissions on alternating trace streams; between two of them a display call writes the Result texture on the main
    stream.  The launch that follows writes the same texture: it must wait for that kernel, and the texture must not have been renamed
    under the pointer the call captured — every frame and the final T0 equal the model."""
    pre, op = writer_into(writer, "T0")
    _, _, marked = overlapped_run(gpu_ctx, models, f"{writer} into the bound Result", pre, [op])
    assert marked["overlapped"] == 0, f"the launch into the texture {writer} has just written does not wait for it"


@pytest.mark.parametrize("writer", WRITERS)
def test_a_display_call_writes_what_is_bound_as_the_sky_and_traced_at_once(gpu_ctx, models, writer):
    pre, op = writer_into(writer, "X1")
    _, _, marked = overlapped_run(gpu_ctx, models, f"{writer} into the next sky", pre, [op, ("bind_sky", "X1")])
    assert marked["overlapped"] == 0, f"the launch that samples what {writer} has just written does not wait for it"


def test_metering_the_result_between_two_submissions(gpu_ctx, models):
    """A reader of the Result texture on the main stream: the state holds the histogram of the frame before it, not of the one after
    (the final state equals the model's), and the launch that overwrites the texture waits.  Control: without the metering the launch
    stays overlapped and every frame is what it is with it."""
    got, _, marked = overlapped_run(gpu_ctx, models, "meter the Result", [], [("meter", "T0", 0, False, 0)])
    assert marked["overlapped"] == 0, "the launch that overwrites the texture being metered does not wait for the metering"
    want = models["meter the Result"]
    assert want[1]["E0"][2] > 0 and want[1]["E0"][0] != 0, "nothing was metered: the protocol proves nothing"
    ops, mark = protocol([("frame", "X0"), ("meter", "T0", 0, False, 0)], after=1)       # (the metering one frame later, in the model)
    assert not cs.same(cs.run_model(ops, profile="display", threads=16, **SHAPE)[1]["E0"], want[1]["E0"]), \
        "the next frame has the same histogram: the protocol proves nothing"
    # control
    ops, mark = protocol([])
    without = run(gpu_ctx, ops, (0, 2), **SHAPE)
    assert dict(without[3])[mark]["overlapped"] == 1, "the launch does not overlap without the metering either"
    assert len(without[0]) == len(got[0]) and all(cs.same(x[2], y[2]) for x, y in zip(without[0], got[0])), "the metering changed a frame"
    assert all(cs.same(without[1][n], got[1][n]) for n in cs.FRAME_TEX), "the metering changed a frame texture"
    assert not without[1]["E0"].any()


def rounds(per_round, n=3):
    """n rounds of a frame and per_round, then a pipelined 8-bit readback of X0 (two tickets in flight)."""
    ops, tickets = [], 0
    for _ in range(n):
        ops += [("frame", None)] + per_round
        if tickets == 2:
            ops.append(("read_end",))
            tickets -= 1
        ops.append(("read_begin", "X0", "RGBA8_SRGB"))
        tickets += 1
    return ops + [("read_end",)] * tickets


def explicit_chain(j):
    return [("meter", "C", 0, False, j), ("bloom", "C", "X0", 0, 3, 0), ("tonemap", "X0", "X0", 0, "aces", 1.0)]


def assert_readbacks_differ(obs, what):
    reads = [a for _, k, a in obs if k == "read_end"]
    assert len(reads) == 3 and all(a.dtype == np.uint8 for a in reads), what
    assert not any(cs.same(reads[a], reads[b]) for a, b in ((0, 1), (0, 2), (1, 2))), f"{what}: two presented frames are the same"


def test_the_presented_frame_chain_with_nothing_waited_for(gpu_ctx, models):
    """frame, meter C at rate 0.25, bloom C -> X0 and tonemap X0 in place with that state, readback — three times, nothing waited for:
    each link reads on the device what the one before it wrote (the state its own previous value, too)."""
    assert cs.METER[1]["rate"] == 0.25
    ops = rounds(explicit_chain(1))
    for cfg, got in run_all(gpu_ctx, models, "presented-frame chain", ops):
        assert_readbacks_differ(got[0], cfg)
        e = got[1]["E0"]
        assert e[0] != e[1] and e[0] != 0, "the exposure sits on its target: the state's history does not show, the protocol proves nothing"


def test_the_master_presents_what_the_explicit_calls_present(gpu_ctx, models):
    """RayTraceMaster.ToneMap with EnableAutoExposure(rate=0.5) and EnableBloom(levels=3) against auto_exposure, bloom and tonemap with
    the same settings: the same bytes, the same state."""
    assert cs.METER[3] == cs.MASTER_EXPOSURE == dict(rate=0.5) and cs.MASTER_BLOOM == dict(levels=3)
    by_master = [("master_bloom", True)] + rounds([("present_tm", "X0", "aces")])
    explicit = rounds(explicit_chain(3))
    a = run_all(gpu_ctx, models, "the master's chain", by_master)
    b = run_all(gpu_ctx, models, "the explicit chain at rate 0.5", explicit)
    for (cfg, x), (_, y) in zip(a, b):
        assert_readbacks_differ(x[0], cfg)
        assert [o[1] for o in x[0]] == [o[1] for o in y[0]] and all(cs.same(p[2], q[2]) for p, q in zip(x[0], y[0])), cfg
        assert cs.same(x[1]["X0"], y[1]["X0"]) and cs.same(x[1]["MS"], y[1]["E0"]) and x[1]["MS"][0] != x[1]["MS"][1], cfg
        assert not y[1]["MS"].any() and not x[1]["E0"].any()


def test_the_bloom_pyramid_regrows_between_deferred_frames(gpu_ctx, models):
    """bloom on the low grid, then on the sky's size, then on the frame's — each needs more scratch than the one before, on a context
    whose scratch has not grown yet — with frames in between and nothing observed until the end."""
    from unityraytracer_amd import Context
    w, h = SHAPE["width"], SHAPE["height"]
    sizes = [cs.low_size(w, h), cs.make_scene(w, h).sky.shape[1::-1], (w, h)]
    texels = [cs.pyramid_texels(*s, 6) for s in sizes]
    assert texels[0] < texels[1] < texels[2], (sizes, texels)
    ops = [("aov_low", False), ("frame", None), ("bloom", "Lc", "Ln", None, 6, 0), ("frame", None), ("bloom", "S0", "S1", None, 6, 0),
           ("frame", None), ("bloom", "C", "X0", None, 6, 0), ("frame", None)]
    want = model_of(models, "pyramid regrow", ops)
    assert all(want[1][n][..., :3].any() for n in ("Ln", "S1", "X0")) and not cs.same(want[1]["X0"], want[1]["C"])
    for cfg in CONFIGS:
        with Context(gpu_ctx.device) as ctx:                     # (a context of its own: its scratch starts empty)
            got = run(ctx, ops, cfg, **SHAPE)
        check(f"pyramid regrow, configuration {cfg} against the model", ops, got, want)
        assert got[2]["watchdog_trips"] == 0, cfg
