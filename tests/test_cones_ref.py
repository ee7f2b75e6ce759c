"""The normal cones of option "blas_cones" (csrc/cones.hip), checked on the host builder's trees through their numpy restatement
(tests/cones_ref.py; tests/test_gpu_cones.py runs the same check on the words read back from the device): whenever the integer test
skips a child for a direction d with | |d| - 1 | <= 2^-10, every triangle below the child has, in float64, d . (e1 x e2) >= 2^-16 |e1| |e2| —
so Moller-Trumbore's back-face culling would have rejected it and the skip cannot change a pixel.  No GPU."""
import numpy as np
import pytest

import cones_ref as K
from unityraytracer_amd import debug_build_blas


def random_directions(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@pytest.fixture(scope="module")
def built(built_library):
    out = {}
    for kind in K.CONE_MESHES:
        sc = K.cone_scene(kind)
        nodes, tri_index, mesh_root, _, _ = debug_build_blas(sc.mesh_objects, sc.vertices, sc.indices)
        _, e1, e2 = K.world_edges(sc, tri_index)
        first, count = K.child_ranges(nodes, mesh_root)
        out[kind] = (nodes, first, count, e1, e2, K.build_cones(nodes, mesh_root, e1, e2))
    return out


@pytest.mark.parametrize("kind", K.CONE_MESHES)
def test_a_skip_means_every_triangle_faces_away(built, kind):
    nodes, first, count, e1, e2, words = built[kind]
    assert (count.sum(axis=1) > 0).all() and len(nodes) > 0
    n_skips, n_cones = K.check_obligation(words, first, count, e1, e2, random_directions(2000, 7))
    assert n_cones > 0 and n_skips > 1000, (n_cones, n_skips)      # not vacuous: cones exist and the test does skip


def test_most_blob_leaves_skip_their_own_axis(built):
    nodes, first, count, e1, e2, words = built["blob"]
    leaf = np.ascontiguousarray(nodes[:, 12:14]).view(np.int32) < 0
    own = K.own_axis_skips(words)
    assert own[leaf].mean() >= 0.5, f"only {own[leaf].mean():.1%} of the blob's leaf children skip the direction along their own axis"
    assert own[~leaf].any()                                          # and interior children have cones too


def test_children_that_cannot_have_a_cone_have_none(built):
    # opposite windings below one child: no cone, at any level
    nodes, first, count, e1, e2, words = built["pair"]
    mixed = 0
    for k in range(len(words)):
        for j in range(2):
            a, b = first[k, j], first[k, j] + count[k, j]
            g = np.cross(e1[a:b].astype(np.float64), e2[a:b].astype(np.float64))
            if (g @ g[0] < 0).any():
                assert words[k, j] == 0, f"node {k} child {j} holds both windings and has a cone"
                mixed += 1
    assert mixed > 0 and (words != 0).any()
    # a zero-area triangle, or one thinner than the margin allows, below a child: no cone
    for kind in ("zero", "slivers"):
        nodes, first, count, e1, e2, words = built[kind]
        g = np.cross(e1.astype(np.float64), e2.astype(np.float64))
        sin_t = np.linalg.norm(g, axis=1) / np.maximum(np.linalg.norm(e1.astype(np.float64), axis=1) * np.linalg.norm(e2.astype(np.float64), axis=1), 1e-300)
        hopeless = sin_t <= K.DELTA
        assert hopeless.any()
        for k in range(len(words)):
            for j in range(2):
                if hopeless[first[k, j]:first[k, j] + count[k, j]].any():
                    assert words[k, j] == 0, f"{kind}: node {k} child {j} covers a triangle that cannot meet the margin and has a cone"
        assert (words != 0).any()


def test_word_zero_and_nan_never_skip():
    d = np.concatenate([random_directions(500, 3), [[np.nan, 0, 1], [0, 0, 0], [np.inf, 0, 0]]]).astype(np.float32)
    assert not K.skips(np.uint32(0), d).any()
    assert K.cone_word(np.array([[np.nan, 0, 0]]), np.array([[0, 1, 0]])) == 0
    assert K.cone_word(np.array([[1.0, 0, 0]]), np.array([[2.0, 0, 0]])) == 0


def test_pack_and_decode_round_trip():
    a = np.array([[-127, 0, 127], [5, -6, 7], [-1, -128, 1]])
    t = np.array([1, 127, -3])
    a2, t2 = K.decode(K.pack(a, t))
    assert np.array_equal(a, a2) and np.array_equal(t, t2)
