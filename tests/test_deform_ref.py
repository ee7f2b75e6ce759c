"""tests/deform_ref.py — the restatement the GPU test of deformed meshes compares the library with — checked on trees small enough to
work out by hand, and the cost's invariance under translation and uniform scale."""
import numpy as np

import deform_ref
from unityraytracer_amd import debug_build_blas, scenes

F = np.float32


def leaf(first, count):
    return np.int32(~((first << 3) | (count - 1)))


def node(lo0, hi0, c0, lo1, hi1, c1):
    n = np.zeros(16, F)
    n[0:3], n[3:6], n[6:9], n[9:12] = lo0, hi0, lo1, hi1
    n[12:14] = np.array([c0, c1], np.int32).view(F)
    return n


def test_cost_of_a_hand_made_two_leaf_tree():
    # one node, two leaves: a 1 x 2 x 3 box holding 4 triangles (area 22) and a 2 x 2 x 2 box holding 1 (area 24); root box 4 x 2 x 3 (area 52)
    nodes = np.stack([node((0, 0, 0), (1, 2, 3), leaf(0, 4), (2, 0, 0), (4, 2, 2), leaf(4, 1))])
    cost, terms = deform_ref.tree_cost(nodes, [0])
    assert terms.tolist() == [2]
    assert cost[0] == (22.0 * 4 + 24.0 * 1) / 52.0
    # a second MeshObject with a root node over a leaf and an interior node: the interior child counts once, whatever lies below it
    inner = node((0, 0, 0), (1, 1, 1), leaf(5, 2), (1, 0, 0), (2, 1, 1), leaf(7, 8))               # areas 6, 6
    top = node((0, 0, 0), (2, 1, 1), np.int32(2), (0, 0, 2), (2, 1, 3), leaf(15, 3))                # areas 10, 10; root box 2 x 1 x 3 (area 22)
    cost, terms = deform_ref.tree_cost(np.stack([nodes[0], top, inner]), [0, 1, np.int32(-2**31)])
    assert terms.tolist() == [2, 4, 0]
    assert cost[0] == 112.0 / 52.0 and cost[1] == (10.0 * 1 + 10.0 * 3 + 6.0 * 2 + 6.0 * 8) / 22.0 and cost[2] == 0.0


def test_non_finite_boxes_add_nothing_and_a_flat_root_costs_nothing():
    inf = np.inf
    nodes = np.stack([node((0, 0, 0), (1, 2, 3), leaf(0, 4), (inf, inf, inf), (-inf, -inf, -inf), leaf(4, 1))])      # an empty child box
    cost, _ = deform_ref.tree_cost(nodes, [0])
    assert cost[0] == 22.0 * 4 / 22.0
    nodes = np.stack([node((0, 0, 0), (1, 2, 3), leaf(0, 4), (np.nan, 0, 0), (1, 1, 1), leaf(4, 1))])
    assert deform_ref.tree_cost(nodes, [0])[0][0] == 4.0
    nodes = np.stack([node((1, 1, 1), (1, 1, 1), leaf(0, 1), (1, 1, 1), (1, 1, 1), leaf(1, 1))])                     # collapsed to a point
    assert deform_ref.tree_cost(nodes, [0])[0][0] == 0.0
    assert deform_ref.tree_cost(np.zeros((0, 16), F), [leaf(0, 2)])[0][0] == 0.0                                      # a single-leaf MeshObject


def test_cost_is_invariant_under_translation_and_uniform_scale():
    sc = scenes.mixed_test_scene(96, 64, blob=(12, 9))
    nodes, tri, root, _, _ = debug_build_blas(sc.mesh_objects, sc.vertices, sc.indices)
    base, terms = deform_ref.tree_cost(nodes, root)
    assert base[0] > 1 and base[1] > 1 and base[2] == 0 and terms[2] == 0            # blob, icosphere; the quad is a single leaf
    for scale, shift in ((1.0, (3.0, -2.0, 7.0)), (4.0, (0, 0, 0)), (0.25, (-1.0, 0.5, 2.0))):     # exact in float32: powers of two, small integers
        moved = np.asarray(nodes, F).copy()
        for a in (0, 3, 6, 9):
            moved[:, a:a + 3] = moved[:, a:a + 3] * F(scale)
        got, _ = deform_ref.tree_cost(moved, root)
        assert np.allclose(got, base, rtol=1e-12, atol=0)
        for a in (0, 3, 6, 9):
            moved[:, a:a + 3] = moved[:, a:a + 3].astype(np.float64) + np.asarray(shift)            # (rounds: the boxes move by up to an ulp)
        got, _ = deform_ref.tree_cost(moved, root)
        assert np.allclose(got, base, rtol=1e-5, atol=0)


def test_span_rule_and_dirty_ranges():
    sc = scenes.mixed_test_scene(96, 64, blob=(12, 9))
    lo, hi = deform_ref.vertex_spans(sc.mesh_objects, sc.indices)
    nv = [12 * 8 + 2, 42, 4]                                                          # blob, icosphere(1), quad: consecutive in _Vertices
    assert lo.tolist() == [0, nv[0], nv[0] + nv[1]] and hi.tolist() == [nv[0] - 1, nv[0] + nv[1] - 1, sum(nv) - 1]
    v = sc.vertices.copy()
    assert deform_ref.dirty_range(sc.vertices, v) is None and not deform_ref.meets((lo, hi), None).any()
    v[nv[0] - 1, 1] += 1
    v[nv[0], 2] += 1
    rng = deform_ref.dirty_range(sc.vertices, v)
    assert rng == (nv[0] - 1, nv[0]) and deform_ref.meets((lo, hi), rng).tolist() == [True, True, False]
    v = sc.vertices.copy(); v[-1, 0] = -0.0 if v[-1, 0] == 0 else -v[-1, 0]            # a sign bit is a change
    assert deform_ref.meets((lo, hi), deform_ref.dirty_range(sc.vertices, v)).tolist() == [False, False, True]
    mo = sc.mesh_objects.copy(); mo[1]["indices_count"] = 2                            # no whole triangle: an empty span meets nothing
    lo2, hi2 = deform_ref.vertex_spans(mo, sc.indices)
    assert lo2[1] > hi2[1] and not deform_ref.meets((lo2, hi2), (0, 10 ** 6))[1]


def test_tri_norms_gather():
    sc = scenes.mixed_test_scene(96, 64, blob=(12, 9))
    _, tri, _, _, _ = debug_build_blas(sc.mesh_objects, sc.vertices, sc.indices)
    tn = deform_ref.tri_norms(sc.normals, sc.indices, tri)
    assert tn.shape == (len(tri), 3, 4) and (tn[:, :, 3] == 0).all()
    k = len(tri) // 2
    for j in range(3):
        assert np.array_equal(tn[k, j, :3], sc.normals[sc.indices[tri[k] + j]])
