"""GPU: program order.  Every API call must behave as if it ran alone, at once, on one stream — whatever the library defers
(csrc/frame_batch.cpp: deferred frames, the blends / presents queued behind them, small launches alternating between two trace streams
behind a narrow dependency).

Fuzz: the random programs of tests/command_stream.py (their reach is held by tests/test_command_stream_model.py).  With nothing deferred
(frames_per_launch 1, overlap_launches 0) a program equals the sequential model bit for bit; every deferring configuration equals that run
bit for bit, radiance queries and the ray counter included.

Directed hazards: a trace launch reads ONE image besides the scene, the sky.  A texture the previous submission wrote — as its present
destination, _converged, the history or the count image, another camera's _target — is bound as _SkyboxTexture and traced at once.  The
launch must wait for that write: launch_info()["overlapped"] == 0 decides it deterministically (a race can pass a pixel comparison by
luck; each protocol runs once).  The control holds the other side: a texture nothing has written keeps the launches overlapped."""
import pytest

import command_stream as cs

pytestmark = pytest.mark.gpu

UNDEFERRED = (1, 0)                                              # (frames_per_launch, overlap_launches)
DEFERRING = ((0, 1), (0, 2), (3, 2), (1, 2))


def check(what, program, got, want, radiance):
    d = cs.first_difference(got, want, radiance)
    if d is not None:
        upto, text = d
        raise AssertionError(f"{what}: {text}\nops{'' if upto is None else ' up to it'}:\n{cs.describe(program, upto)}")


@pytest.mark.parametrize("seed", range(24))
def test_random_programs_keep_program_order(gpu_ctx, seed):
    program = cs.make_program(seed)
    model = cs.run_model(program)
    plain = cs.run_gpu(gpu_ctx, program, *UNDEFERRED)
    check(f"seed {seed}, configuration {UNDEFERRED} against the model", program, plain, model, radiance=False)
    assert plain[2]["watchdog_trips"] == 0
    for cfg in DEFERRING:
        got = cs.run_gpu(gpu_ctx, program, *cfg)
        check(f"seed {seed}, configuration {cfg} against {UNDEFERRED}", program, got, plain, radiance=True)
        assert got[2]["rays"] == plain[2]["rays"], (seed, cfg, got[2]["rays"], plain[2]["rays"])
        assert got[2]["dispatches"] == plain[2]["dispatches"] and got[2]["launches"] <= plain[2]["launches"], (seed, cfg)
        assert got[2]["watchdog_trips"] == 0, (seed, cfg)


# ---- directed hazards ----------------------------------------------------------------------------------------------------------------
SHAPE = dict(width=200, height=120, bounces=6)                   # the shape of tests/test_gpu_overlap.py: a launch outlasts a blend


def protocol(bind, history=False, before=2, after=2, dest_after="X0"):
    """One-frame submissions (frame, present into X0, pipelined readback of it — two tickets in flight): `before` of them, the `bind` ops,
    `after` more, presented into `dest_after` (without the history blend: it is refused while H or N is the sky).  -> (ops, index of the
    first readback after the bind: launch_info() there describes the launch that follows the bind)."""
    ops, tickets, mark = [], 0, None
    for n in range(before + after):
        if n == before:
            ops += bind
        dest = "X0" if n < before else dest_after
        ops.append(("frame", dest))
        if history and n < before:
            ops.append(("history", 0.0))
        if tickets == 2:
            ops.append(("read_end",))
            tickets -= 1
        ops.append(("read_begin", dest, "RGBA32F"))
        tickets += 1
        if n == before:
            mark = len(ops) - 1
    ops += [("read_end",)] * tickets
    return ops, mark


CASES = {
    "present destination": (protocol([("bind_sky", "X0")], dest_after="X1"), False),
    "_converged": (protocol([("bind_sky", "C")]), False),
    "history image": (protocol([("bind_sky", "H")], history=True), False),
    "count image": (protocol([("bind_sky", "N")], history=True), False),
    "another camera's _target": (protocol([("bind_result",), ("bind_sky", "T0")]), True),
}


def launches(infos, ops):
    """launch_info() after each readback's submission, in order."""
    return [info for (i, info) in infos if ops[i][0] == "read_begin"]


@pytest.fixture(scope="module")
def models():
    """The sequential model of each protocol, made once."""
    return {}


def run_directed(gpu_ctx, models, name, ops):
    if name not in models:
        models[name] = cs.run_model(ops, threads=16, **SHAPE)
    got = cs.run_gpu(gpu_ctx, ops, 0, 2, **SHAPE)
    plain = cs.run_gpu(gpu_ctx, ops, *UNDEFERRED, **SHAPE)
    check(f"{name}: undeferred against the model", ops, plain, models[name], radiance=False)
    check(f"{name}: overlapped against undeferred", ops, got, plain, radiance=True)
    assert got[2]["watchdog_trips"] == 0 and plain[2]["watchdog_trips"] == 0
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_sky_written_by_the_previous_submission(gpu_ctx, models, name):
    (ops, mark), wrap = CASES[name]
    got = run_directed(gpu_ctx, models, name, ops)
    infos = dict(got[3])
    ls = launches(got[3], ops)
    assert all(i["n_frames"] == 1 and i["trace_stream"] in (1, 2) for i in ls), ls          # one-frame submissions on the trace streams
    assert ls[1]["overlapped"] == 1, "the undisturbed second launch does not overlap: the protocol shows nothing"
    assert infos[mark]["overlapped"] == 0, f"{name}: the launch that samples it does not wait for the write"
    if not wrap:
        return
    # once more with the slot cursor at the end of the slab: the launch into T0 takes the last slot, the one that samples T0 wraps to slot 0
    slots, cursor = ls[-1]["slab_frames"], ls[-1]["slab_base"] + 1
    skip = (slots - 2 - cursor) % slots
    advance = ([("frame", None)] * 8 + [("flush",)]) * (skip // 8) + [("frame", None), ("flush",)] * (skip % 8)     # launches of <= 8 frames take part
    cs.run_gpu(gpu_ctx, advance, 0, 2, **dict(SHAPE, bounces=1))
    got = run_directed(gpu_ctx, models, name, ops)
    ls = launches(got[3], ops)
    assert [i["slab_base"] for i in ls[:3]] == [slots - 2, slots - 1, 0], [i["slab_base"] for i in ls]
    assert dict(got[3])[mark]["overlapped"] == 0


def test_control_an_unwritten_sky_keeps_the_overlap(gpu_ctx, models):
    """Binding a texture nothing has written since the last widened launch is no reason to wait: a fix that always widens fails here."""
    ops, mark = protocol([("bind_sky", "X2")], before=3, after=3)
    got = run_directed(gpu_ctx, models, "control", ops)
    ls = launches(got[3], ops)
    assert dict(got[3])[mark]["overlapped"] == 1
    assert [i["overlapped"] for i in ls] == [0, 1, 1, 1, 1, 1], ls
    assert [i["trace_stream"] for i in ls] in ([1, 2, 1, 2, 1, 2], [2, 1, 2, 1, 2, 1]), ls
    # ... and in the hazard protocols the launch AFTER the widened one overlaps again where nothing writes the sky any more
    (ops, mark), _ = CASES["present destination"]
    got = cs.run_gpu(gpu_ctx, ops, 0, 2, **SHAPE)
    assert [i["overlapped"] for i in launches(got[3], ops)][-1] == 1
