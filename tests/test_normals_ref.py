"""CPU: the restatement of the normals on the device (tests/normals_ref.py) against what exists — host_scene.compute_normals
(csrc/host_scene.cpp, which now shares its grouping with the plan: csrc/normals_plan.cpp) and scenes.compute_normals — and the canonical
plan of urt_debug_build_normals_plan against the restatement's, exactly.  Bit for bit throughout: uint32 equality."""
import ctypes as C

import numpy as np
import pytest

import normals_ref as N
from unityraytracer_amd import _lib, host_scene, scenes

F = np.float32
SCENE = 8


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("name", sorted(N.MESHES))
def test_restatement_at_rest_equals_the_host(built_library, name):
    v, t = N.MESHES[name]()
    got = N.compute_normals(v, t)
    assert np.array_equal(bits(got), bits(host_scene.compute_normals(v, t))), name
    with np.errstate(all="ignore"):
        plain = scenes.compute_normals(v, t)
    # scenes.compute_normals welds by plain equality (its docstring says so): the rows of the vertices that have a PARTNER are the ones it
    # cannot give, and only the mesh built for that rule has any (vertices 0, 2, 3, 4, 5, 6 of partner_case)
    partnered = np.zeros(len(v), bool)
    if name == "partner":
        partnered[[0, 2, 3, 4, 5, 6]] = True
        assert (bits(got[partnered]) != bits(plain[partnered])).any(axis=1).all()
    assert np.array_equal(bits(got[~partnered]), bits(plain[~partnered])), name


def test_the_special_vertices_get_what_the_reference_gives_them(built_library):
    v, t = N.odd_ones()
    n = N.compute_normals(v, t)
    assert (bits(n[4:8]) == 0).all()                        # the degenerate triangle's corners and the unreferenced vertex: +0
    p = N.plan(v, t)
    assert p["ranges"][7, 1] == 0
    lst = p["entries"][p["ranges"][8, 0]: p["ranges"][8, 0] + p["ranges"][8, 1]]
    assert np.array_equal(p["ranges"][8], p["ranges"][9]) and sorted(lst.tolist()).count(int(lst[0])) == 2      # one triangle, two slots
    v, t = N.partner_case()
    p = N.plan(v, t)
    assert p["ranges"][:7, 1].tolist() == [3, 1, 3, 3, 2, 3, 2]                              # (the docstring of partner_case)
    assert np.array_equal(p["ranges"][0], p["ranges"][2]) and not np.array_equal(p["ranges"][0], p["ranges"][3])   # equal shares, a partner does not
    n = N.compute_normals(v, t)
    assert np.array_equal(bits(n[0]), bits(n[3])) and np.array_equal(bits(n[0]), bits(n[2])) and not np.array_equal(bits(n[0]), bits(n[1]))
    assert not np.array_equal(bits(n[4]), bits(n[6]))                                        # not transitive
    v, t = N.cube24()
    p = N.plan(v, t)
    assert p["n_lists"] == 8 and len(p["tris"]) == 12 and len(p["entries"]) == 36


@pytest.mark.parametrize("name", ["mixed", "cube24", "seam_sphere", "two_quads", "odd_ones"])
def test_a_rest_plan_serves_deformations_that_keep_the_weld(built_library, name):
    v, t = N.MESHES[name]()
    p = N.plan(v, t)
    for phase in (0.0, 1.1, 2.9):
        w = N.wobble(v, phase)
        assert N.welds_alike(v, w, t), (name, phase)        # a condition on the inputs
        want = host_scene.compute_normals(w, t)
        assert np.array_equal(bits(N.apply(p, w)), bits(want)), (name, phase)
        assert (bits(want) != bits(host_scene.compute_normals(v, t))).any()


def test_a_deformation_that_splits_a_weld_is_told_apart():
    v, t = N.two_quads()
    w = v.copy()
    w[4] += F(0.25)                                          # one of the two coincident pairs comes apart
    assert not N.welds_alike(v, w, t)


@pytest.mark.parametrize("name,first,count", [("mixed", 0, 98), ("mixed", 98, 42), ("mixed", 140, 4), ("two_quads", 0, 4), ("two_quads", 4, 4),
                                              ("seam_sphere", 5, 17), ("odd_ones", 7, 3), ("partner", 3, 3), ("cube24", 0, 0)])
def test_a_sub_span_plan_equals_the_rows_of_the_whole(built_library, name, first, count):
    v, t = N.MESHES[name]()
    whole = host_scene.compute_normals(v, t)
    p = N.plan(v, t, first, count)
    assert np.array_equal(bits(N.apply(p, v)), bits(whole[first: first + count]))
    if name == "two_quads":                                  # the neighbour's triangles along the shared edge are needed
        assert len(p["tris"]) == 4


def native_plan(v, t, first, count):
    p = host_scene.normals_plan(v, t, first, count)
    return p["ranges"], p["entries"], p["tris"], p["max_valence"]


@pytest.mark.parametrize("name", sorted(N.MESHES))
def test_the_native_plan_equals_the_restatement(built_library, name):
    v, t = N.MESHES[name]()
    spans = [(0, len(v)), (1, len(v) - 2), (len(v) // 2, 1), (len(v), 0), (0, 0)]
    for first, count in spans:
        want = N.plan(v, t, first, count)
        ranges, entries, tris, valence = native_plan(v, t, first, count)
        what = (name, first, count)
        assert np.array_equal(ranges, want["ranges"]), what
        assert np.array_equal(entries, want["entries"]), what
        assert np.array_equal(tris, want["tris"]), what
        assert valence == want["max_valence"], what


def test_size_queries_and_errors(built_library):
    lib = _lib.load()
    v, t = N.seam_sphere()
    want = N.plan(v, t, 2, 9)
    vp, tp = v.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p)
    sizes = (C.c_int32 * 3)()
    assert lib.urt_debug_build_normals_plan(vp, len(v), tp, t.size, 2, 9, None, None, 0, None, 0, sizes) == 0
    assert list(sizes) == [len(want["entries"]), len(want["tris"]), want["max_valence"]]
    assert lib.urt_debug_build_normals_plan(vp, len(v), tp, t.size, 2, 9, None, None, 0, None, 0, None) == 0
    entries = np.zeros(sizes[0], np.int32)
    ep = entries.ctypes.data_as(C.c_void_p)
    assert lib.urt_debug_build_normals_plan(vp, len(v), tp, t.size, 2, 9, None, ep, sizes[0], None, 0, None) == 0
    assert np.array_equal(entries, want["entries"])
    assert lib.urt_debug_build_normals_plan(vp, len(v), tp, t.size, 2, 9, None, ep, sizes[0] - 1, None, 0, None) == 1      # too small
    for first, count in ((-1, 1), (0, -1), (len(v), 1), (2 ** 31 - 1, 2)):
        assert lib.urt_debug_build_normals_plan(vp, len(v), tp, t.size, first, count, None, None, 0, None, 0, sizes) == 1
    assert lib.urt_debug_build_normals_plan(vp, len(v), tp, t.size - 1, 0, 1, None, None, 0, None, 0, sizes) == 1           # not triangles
    assert lib.urt_debug_build_normals_plan(None, len(v), tp, t.size, 0, 1, None, None, 0, None, 0, sizes) == 1
    for bad in (len(v), -1):
        t2 = t.copy()
        t2[-2] = bad
        rc = lib.urt_debug_build_normals_plan(vp, len(v), t2.ctypes.data_as(C.c_void_p), t2.size, 0, 1, None, None, 0, None, 0, sizes)
        assert rc == SCENE and b"index outside" in lib.urt_host_last_error()
        with pytest.raises(_lib.UrtError):
            host_scene.normals_plan(v, t2)
