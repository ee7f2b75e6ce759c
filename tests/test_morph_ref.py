"""tests/morph_ref.py — the numpy restatement of include/urt.h urt_morph_vertices and of the canonical morph plan — against float64
morphing within a derived bound and on hand-made cases, and the library's host-side plan builder (urt_debug_build_morph_plan,
csrc/morph_plan.cpp) against the restated plan, array for array.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import morph_ref as M
from unityraytracer_amd import _lib, host_scene
from unityraytracer_amd._lib import UrtError

F = np.float32
INVALID_ARGUMENT, SCENE = 1, 8


def random_case(seed, count, first, n_targets, n_deltas, duplicates=True):
    rng = np.random.default_rng(seed)
    n = first + count + 3
    P = rng.uniform(-3, 3, (n, 3)).astype(F)
    N = rng.normal(size=(n, 3)).astype(F)
    vertex = rng.integers(first, first + count, n_deltas)
    target = rng.integers(0, n_targets, n_deltas)
    if duplicates and n_deltas > 4:                          # the same (vertex, target) pair several times, apart in the input
        vertex[-3:], target[-3:] = vertex[0], target[0]
    d = M.deltas_array(vertex, target, rng.uniform(-1, 1, (n_deltas, 3)), rng.uniform(-1, 1, (n_deltas, 3)))
    w = rng.uniform(-1.5, 1.5, n_targets).astype(F)
    w[rng.random(n_targets) < 0.4] = 0
    return P, N, d, w


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,n_targets,n_deltas", [(1, 1, 7), (65, 3, 400), (300, 40, 5000)])
def test_the_restatement_is_float64_morphing_within_the_derived_bound(count, n_targets, n_deltas):
    for first in (0, 5):
        P, N, d, w = random_case(17 * count + first, count, first, n_targets, n_deltas)
        got, _ = M.morph(P, N, d, first, count, w)
        want, bound = M.morph64(P, d, first, count, w)
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= bound).all(), (count, first, float((err - bound).max()))
        assert bound.max() < 1e-3                            # (small against the deltas: the comparison means something)


def test_a_vertex_without_a_live_entry_keeps_its_rest_pose_bit_for_bit():
    P = np.array([[1.5, -0.0, 3.25], [-0.0, -0.0, -0.0], [7, 8, 9]], F)
    N = np.array([[0, 0, 2], [-0.0, 0, 0], [0, 3, 4]], F)
    d = M.deltas_array([0, 1, 1, 0], [0, 0, 1, 1], [[1, 1, 1], [5, 5, 5], [np.inf, -np.inf, np.nan], [np.inf, 0, 0]], [[1, 0, 0]] * 4)
    p, n = M.morph(P, N, d, 0, 3, np.zeros(2, F))            # every entry dead
    assert p.tobytes() == P.tobytes() and n.tobytes() == N.tobytes()       # -0.0 stays -0.0, inf * 0 makes no NaN
    p, n = M.morph(P, N, d, 0, 3, np.zeros(2, F), normalize=True)
    assert p.tobytes() == P.tobytes()
    assert n[0].tolist() == [0, 0, 1] and n[1].tobytes() == N[1].tobytes() and np.allclose(n[2], [0, 0.6, 0.8], atol=1e-7)    # L2 == 0: as it is


def test_the_live_rule_by_hand():
    P = np.array([[1, 2, 3], [0, 0, 0]], F)
    N = np.array([[0, 0, 1], [0, 1, 0]], F)
    d = M.deltas_array([0, 0, 1, 0], [1, 0, 0, 1], [[1, 0, 0], [0, 10, 0], [1, 1, 1], [0.5, 0, 0]], [[0, 0, 0]] * 4)
    # vertex 0: plan order is target 0 (input 1), then target 1 twice in input order (inputs 0 and 3)
    ranges, order, sizes = M.plan(d, 0, 2)
    assert order.tolist() == [1, 0, 3, 2] and ranges.tolist() == [[0, 3], [3, 1]] and sizes == (4, 3, 2)
    p, _ = M.morph(P, N, d, 0, 2, np.array([0.5, 2.0], F))
    assert p.tolist() == [[1 + 2.0 + 1.0, 2 + 5.0, 3], [0.5, 0.5, 0.5]]
    p, _ = M.morph(P, N, d, 0, 2, np.array([0.0, 2.0], F))   # target 0 dead
    assert p.tolist() == [[4, 2, 3], [0, 0, 0]]
    # a negative zero weight is zero: dead.  A NaN weight is live and poisons what it touches, and only that.
    p, _ = M.morph(P, N, d, 0, 2, np.array([-0.0, np.nan], F))
    assert np.isnan(p[0]).all() and p[1].tolist() == [0, 0, 0]       # (NaN * 0 is NaN too: all three components of vertex 0)
    # the sum is sequential in plan order: a large term, then its opposite, then a small one — and not the other way round
    big = M.deltas_array([0, 0, 0], [0, 1, 2], [[1e8, 0, 0], [-1e8, 0, 0], [1, 0, 0]])
    p, _ = M.morph(np.array([[1, 0, 0]], F), None, big, 0, 1, np.ones(3, F))
    assert p[0, 0] == 1.0                                     # ((1 + 1e8) - 1e8) + 1 in float32: the first 1 is lost, the last one stays
    # positions only
    assert M.morph(P, None, d, 0, 2, np.ones(2, F))[1] is None


def test_normalize_follows_the_rule_of_skinning():
    N = np.array([[3, 0, 4], [0, 0, 0], [1e30, 1e30, 0], [np.nan, 0, 0]], F)
    d = M.deltas_array([], [], np.zeros((0, 3)))
    _, n = M.morph(np.zeros((4, 3), F), N, d, 0, 4, np.zeros(1, F), normalize=True)
    assert np.allclose(n[0], [0.6, 0, 0.8], atol=1e-7)
    assert n[1:3].tobytes() == N[1:3].tobytes() and np.isnan(n[3, 0]) and n[3, 1:].tolist() == [0, 0]      # L2 zero, infinite, NaN: as it is


# ---- the plan builder of the library ------------------------------------------------------------------------------------------------
def lib_plan(d, n_targets, first, count):
    return host_scene.morph_plan(d, n_targets, first, count)


@pytest.mark.parametrize("count,first,n_targets,n_deltas", [(1, 0, 1, 9), (40, 0, 5, 300), (40, 7, 5, 300), (500, 3, 300, 20), (257, 0, 4096, 3000),
                                                            (12, 4, 2, 0), (0, 9, 3, 0)])
def test_the_library_builds_the_restated_plan(built_library, count, first, n_targets, n_deltas):
    _, _, d, _ = random_case(count + n_deltas, max(count, 1), first, n_targets, n_deltas)
    if count == 0:
        d = d[:0]
    got = lib_plan(d, n_targets, first, count)
    ranges, order, (n_entries, max_valence, n_touched) = M.plan(d, first, count)
    assert np.array_equal(got["order"], order) and np.array_equal(got["ranges"], ranges)
    assert (got["n_entries"], got["max_valence"], got["n_touched"]) == (n_entries, max_valence, n_touched)
    assert got["ranges"].dtype == np.int32 and got["order"].dtype == np.int32
    if count == 500:
        assert (ranges[:, 1] == 0).sum() > 400               # vertices of valence 0 between the touched ones
        assert n_touched < 21


def test_nothing_is_pruned_and_duplicates_stay_in_input_order(built_library):
    d = M.deltas_array([6, 5, 6, 6, 5, 6], [1, 0, 1, 0, 0, 1], np.zeros((6, 3)))        # all-zero deltas, (6, 1) three times, (5, 0) twice
    got = lib_plan(d, 2, 5, 3)
    assert got["order"].tolist() == [1, 4, 3, 0, 2, 5] and got["ranges"].tolist() == [[0, 2], [2, 4], [6, 0]]
    assert (got["n_entries"], got["max_valence"], got["n_touched"]) == (6, 4, 2)
    # the tuple form of host_scene.morph_deltas is the same array
    again = lib_plan([(int(r["vertex"]), int(r["target"]), r["dp"], r["dn"]) for r in d], 2, 5, 3)
    assert again["order"].tolist() == got["order"].tolist()


def test_the_plan_builders_error_codes(built_library):
    lib = _lib.load()
    d = M.deltas_array([3, 4], [0, 1], np.ones((2, 3)))
    ranges, order, sizes = np.full((2, 2), 77, np.int32), np.full(2, 77, np.int32), np.full(3, 77, np.int32)

    def call(deltas=d, n_deltas=2, n_targets=2, first=3, count=2, r=ranges, o=order, s=sizes):
        p = (lambda a: None if a is None else a.ctypes.data_as(C.c_void_p))
        return lib.urt_debug_build_morph_plan(p(deltas), n_deltas, n_targets, first, count, p(r), p(o), p(s))

    assert call(deltas=None) == INVALID_ARGUMENT
    assert call(n_deltas=-1) == INVALID_ARGUMENT and call(count=-1) == INVALID_ARGUMENT and call(first=-1) == INVALID_ARGUMENT
    assert call(first=2 ** 31 - 1, count=2) == INVALID_ARGUMENT
    for n_targets in (0, -1, 4097, 2 ** 31 - 1):
        assert call(n_targets=n_targets) == INVALID_ARGUMENT, n_targets
    assert call(first=4) == SCENE and call(count=1) == SCENE and call(first=0, count=4) == SCENE      # a vertex outside the served range
    assert call(n_targets=1) == SCENE                                                                  # a target outside 0..n_targets-1
    bad = d.copy(); bad["target"][0] = -1
    assert call(deltas=bad) == SCENE
    assert call(n_deltas=1, count=0) == SCENE                # nothing is served: every vertex is outside
    assert (ranges == 77).all() and (order == 77).all() and (sizes == 77).all()          # an error writes nothing
    assert b"morph plan" in lib.urt_host_last_error()
    with pytest.raises(UrtError):
        host_scene.morph_plan(d, 1, 3, 2)
    # legal: no deltas, nothing served, NULL outputs, the largest target table
    assert call(deltas=None, n_deltas=0) == 0 and sizes.tolist() == [0, 0, 0] and ranges.tolist() == [[0, 0], [0, 0]]
    assert call(deltas=None, n_deltas=0, count=0, r=None, o=None, s=None) == 0
    assert call(r=None, o=None, s=None) == 0 and call(n_targets=4096) == 0
    assert call() == 0 and order.tolist() == [0, 1] and ranges.tolist() == [[0, 1], [1, 1]] and sizes.tolist() == [2, 1, 2]
