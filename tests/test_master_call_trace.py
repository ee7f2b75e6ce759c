"""RayTraceMaster sends the library exactly the calls it sent before its host-side refactoring: the script of tests/master_trace.py
(every edit with and without history, the device-side paths, the queries, the image-space stages, a resize, edits before the trees exist)
on a recording stand-in for the library, compared record for record with tests/golden/master_call_trace.json, which was made from the
commit before the refactoring (the command is in master_trace's docstring).  No tolerance: names, order, handles, scalars and the digests
of every host array.  Auto-exposure: an opaque state is injected instead of EnableAutoExposure's tensor (see master_trace).  No GPU."""
import json
import os

import pytest

import master_trace

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "master_call_trace.json")
EDITS = ("MoveCamera", "MoveObjects", "DeformMeshes", "SkinMeshes", "MorphMeshes")      # (the last two share _deform_on_device)


@pytest.fixture(scope="module")
def trace(built_library):
    return json.loads(master_trace.dumps(master_trace.run()))      # through the writer: what a regenerated fixture would hold


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def first_difference(got, want, arrays_got, arrays_want):
    """None, or a message that names the first record that differs and the step of the script it belongs to."""
    def full(r, arrays):                                           # "@k" -> the array's description: two tables may number them differently
        if isinstance(r, list):
            return [full(x, arrays) for x in r]
        if isinstance(r, dict):
            return {k: full(v, arrays) for k, v in r.items()}
        return arrays[int(r[1:])] if isinstance(r, str) and r[:1] == "@" and r[1:].isdigit() else r
    step = "the start"
    for k in range(max(len(got), len(want))):
        g = full(got[k], arrays_got) if k < len(got) else "nothing (the trace ends)"
        w = full(want[k], arrays_want) if k < len(want) else "nothing (the trace ends)"
        if g != w:
            return f"record {k}, after {step!r}:\n  expected {json.dumps(w)}\n  got      {json.dumps(g)}"
        if isinstance(w, list) and w[0] == "#":
            step = w[1]
    return None


@pytest.mark.parametrize("name", [name for name, _ in master_trace.RUNS])
def test_the_calls_are_those_of_the_commit_before_the_refactoring(trace, golden, name):
    assert first_difference(trace["runs"][name], golden["runs"][name], trace["arrays"], golden["arrays"]) is None
    assert trace["runs"][name] == golden["runs"][name]


def test_the_whole_trace_is_the_fixture(trace, golden):
    assert list(trace["runs"]) == list(golden["runs"]) == [name for name, _ in master_trace.RUNS]
    assert trace == golden
    with open(GOLDEN) as f:
        assert f.read() == master_trace.dumps(trace)               # byte for byte what the generator writes


def test_a_difference_is_reported_with_its_step():
    want = [["#", "MoveCamera x"], ["urt_blit", "T0", "T1"], ["urt_shader_set_matrix", "m", "@0"]]
    arrays = [{"shape": [16], "dtype": "float32", "sha256": "aa"}, {"shape": [16], "dtype": "float32", "sha256": "bb"}]
    assert first_difference(want, want, arrays, arrays) is None
    message = first_difference(want[:2] + [["urt_shader_set_matrix", "m", "@1"]], want, arrays, arrays)
    assert message.startswith("record 2, after 'MoveCamera x'") and '"bb"' in message and '"aa"' in message
    assert "the trace ends" in first_difference(want[:2], want, arrays, arrays)
    assert first_difference(want, want, arrays, arrays[::-1]) is not None


def test_every_reachable_entry_point_is_in_the_trace(golden):
    seen = {r[0] for records in golden["runs"].values() for r in records}
    assert [name for name in master_trace.REACHABLE if name not in seen] == []
    assert seen - {"#"} <= set(master_trace.REACHABLE)
    assert all(name.startswith("urt_") for name in master_trace.REACHABLE)


def test_every_edit_took_both_its_branches(golden):
    plain, temporal = master_trace.branches(golden["runs"]["plain"]), master_trace.branches(golden["runs"]["temporal"])
    for edit in EDITS:
        assert plain[edit] == {False}, edit                        # temporal accumulation off: nothing is ever reprojected
        assert temporal[edit] == {True, False}, edit               # on: with history, and without (before the trees exist, after a resize)
    kinds = {r[0] for r in golden["runs"]["temporal"]}
    assert set(master_trace.REPROJECTS) <= kinds                   # MoveCamera's entry point, the objects' and the deformed meshes'
