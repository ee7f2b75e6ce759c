"""The numpy restatement of the GPU triangle-BVH builders (tests/lbvh_ref.py) is checked here before tests/test_gpu_lbvh_exact.py
trusts it: against the host builder, which is independent C++ (csrc/blas_builder.cpp), as a set of nodes bit for bit; in float64 and
exactly, on every builder's tree, for the properties a BVH of these builders has (boxes contain, boxes are TIGHT, no interior node
over a leaf's worth of triangles, builder 2 within its depth budget); and with negative controls — variants of the restatement that
differ in one decision must each change a tree of the GPU test's scenes, or those scenes could not see that decision go wrong."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

import lbvh_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_host = {}


def host_trees(leaf_max):
    """debug_build_blas of every scene of L.HOST_SCENES with `leaf_max` triangles per leaf.  The host builder reads its leaf size when the
    library is loaded (URT_BLAS_LEAF_MAX), so it runs in a process of its own."""
    if leaf_max not in _host:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "host.npz")
            code = ("import sys; sys.path[:0] = [%r, %r]\n"
                    "import numpy as np, lbvh_ref as L\n"
                    "from unityraytracer_amd import debug_build_blas\n"
                    "out = {}\n"
                    "for name in L.HOST_SCENES:\n"
                    "    sc = L.GPU_SCENES[name]()\n"
                    "    n, t, r, _, d = debug_build_blas(sc.mesh_objects, sc.vertices, sc.indices)\n"
                    "    out.update({name + '.nodes': n, name + '.tri': t, name + '.root': r, name + '.depth': np.int64(d)})\n"
                    "np.savez(%r, **out)\n") % (ROOT, os.path.join(ROOT, "tests"), path)
            subprocess.run([sys.executable, "-c", code], env=dict(os.environ, URT_BLAS_LEAF_MAX=str(leaf_max)), check=True)
            with np.load(path) as z:
                _host[leaf_max] = {k: z[k] for k in z.files}
    return _host[leaf_max]


# uv_blob meshes have pairs of triangles with one centroid at their poles: with one triangle per leaf the last split of such a pair
# is a positional halving, so those scenes qualify for the comparison at 2 and 4 triangles per leaf only; the icosphere scenes at 1 too
HOST_CASES = [(n, lm) for n in L.HOST_SCENES for lm in (1, 2, 4) if lm > 1 or n.startswith("many")]


@pytest.mark.parametrize("name,leaf_max", HOST_CASES)
def test_sah_restatement_with_32_bins_is_the_host_builders_tree(built_library, name, leaf_max):
    """Builder 3 restated with 32 bins at every size gives the host builder's tree as a SET of nodes: for every interior node the index
    slots below child 0 and below child 1 and the 12 box floats bit for bit, and the same multiset of leaves (the host numbers depth-first
    and partitions unstably).  Only where the restatement never halves by position (asserted): halving depends on the order."""
    sc = L.GPU_SCENES[name]()
    ref = L.build_sah(sc, leaf_max, small_bins=32)
    assert ref["n_halved"] == 0, "the comparison is defined only without the positional-halving fallback"
    h = host_trees(leaf_max)
    hn, ht, hr = h[name + ".nodes"], h[name + ".tri"], h[name + ".root"]
    assert leaf_max == 2 or not np.array_equal(hn, host_trees(2)[name + ".nodes"])       # (the leaf size reached the host builder)
    mine, host = L.canonical(ref["nodes"], ref["tri_index"], ref["mesh_root"]), L.canonical(hn, ht, hr)
    assert len(mine[0]) == len(hn) == ref["n_nodes"]
    assert mine[0] == host[0], f"{len(mine[0] - host[0])} interior nodes differ"
    assert mine[1] == host[1]
    assert ref["max_depth"] == int(h[name + ".depth"])
    cost, host_cost = L.sah_cost(ref["nodes"], ref["mesh_root"]), L.sah_cost(hn, hr)
    real = L.build_sah(sc, leaf_max)
    print(f"{name} leaf_max {leaf_max}: surface-area cost {cost!r} (32 bins, = host), {L.sah_cost(real['nodes'], real['mesh_root'])!r} (8 / 32 bins), "
          f"{ref['n_nodes']} / {real['n_nodes']} nodes")
    assert cost == host_cost                                                               # to the last bit


ORDINARY = ("mixed", "many70", "many70_level1", "many120", "c3_5520", "thresholds")


@pytest.mark.parametrize("builder", [1, 2, 3])
@pytest.mark.parametrize("name", [n for n in L.GPU_SCENES if n != "c3_69600"] + ["non_finite", "empty_and_tiny"])
def test_restated_trees_hold_and_are_tight(name, builder):
    for leaf_max in (1, 2, 4, 8) if name in ("mixed", "thresholds", "degenerate") else (2,):
        sc = empty_and_tiny_scene() if name == "empty_and_tiny" else L.nonfinite_scene() if name == "non_finite" else L.GPU_SCENES[name]()
        for slack in (0, 6) if builder == 2 else (6,):
            t = L.build(sc, builder, leaf_max, slack)
            res = L.check_tree(sc, t, leaf_max)
            loose = res.pop("loose")
            assert not any(res.values()), (name, builder, leaf_max, slack, res)
            if builder == 3:
                assert loose <= 2 * t["n_halved"]
                if name in ORDINARY and (leaf_max > 1 or name.startswith("many")):       # (HOST_CASES: coincident centroids at a blob's poles)
                    assert t["n_halved"] == 0 and loose == 0, (name, t["n_halved"])
            else:
                assert loose == 0
            if builder == 2:
                assert t["max_depth"] <= t["depth_cap"], (name, leaf_max, slack)
            # leaves hold 1 .. leaf_max triangles, interior roots are nodes 0 .. k-1 in MeshObject order
            codes = np.concatenate([t["nodes"][:, 12:14].view(np.int32).reshape(-1), t["mesh_root"][t["mesh_root"] != L.EMPTY_ROOT]])
            assert (L.leaf_range(codes[codes < 0])[1] <= leaf_max).all()
            roots = [int(r) for r in t["mesh_root"] if 0 <= r != L.EMPTY_ROOT]
            assert roots == list(range(len(roots)))


def empty_and_tiny_scene():
    """MeshObjects of 0, 1, 2 and 9 triangles around an ordinary one: the roots that are no nodes."""
    from unityraytracer_amd import scenes
    v, t = scenes.uv_blob(12, 9)
    t = np.asarray(t, np.int32).reshape(-1, 3)
    b = scenes.MeshSceneBuilder()
    mat = scenes._params((0.7, 0.6, 0.5), (0.1, 0.1, 0.1), (0, 0, 0), 0.4)
    for k, n in enumerate((1, 2, len(t), 9)):
        b.add(v, t[:n], scenes.trs(translate=(k - 2.0, 1.0, 1.0)), mat)
    sc = L._scene("empty-and-tiny", b)
    mo = sc.mesh_objects
    empty = mo[[1, 3]].copy()                      # (a scene for the restatement only: its object-level heap does not know the empty ones)
    empty["indices_count"] = 0
    sc.mesh_objects = np.concatenate([mo[:1], empty[:1], mo[1:3], empty[1:], mo[3:]])
    return sc


def test_roots_that_are_no_nodes():
    sc = empty_and_tiny_scene()
    for builder in (1, 2, 3):
        t = L.build(sc, builder, 2)
        r = t["mesh_root"]
        assert r[1] == r[4] == 0x7FFFFFFF and r[0] == ~np.int32(0) and r[2] == ~np.int32((1 << 3) | 1) and r[3] == 0 and r[5] == 1
        assert L.build(sc, builder, 8)["mesh_root"][2] == ~np.int32((1 << 3) | 1)


def test_conversions_and_order_images():
    """The float -> int rule (towards zero, saturating, NaN -> 0) and the order-preserving images (-0 below +0, round trip exact)."""
    x = np.array([np.nan, -np.inf, -3e9, -1.5, -0.0, 0.0, 0.99, 31.999, 3e9, np.inf], np.float32)
    assert L.f2i(x).tolist() == [0, -2147483648, -2147483648, -1, 0, 0, 0, 31, 2147483647, 2147483647]
    f = np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32)
    o = L.f2ord(f)
    assert (np.diff(o.astype(np.int64)) > 0).all() and np.array_equal(L.ord2f(o).view(np.uint32), f.view(np.uint32))
    a = np.array([[3.0, 1e-3, 7.0]], np.float32)
    assert L.half_area(np.zeros((1, 3), np.float32), a)[0] == np.float32(np.float32(np.float32(3.0) * np.float32(1e-3)) + np.float32(np.float32(1e-3) * np.float32(7.0))) + np.float32(21.0)


def differs(a, b):
    return not (np.array_equal(a["nodes"].view(np.uint32), b["nodes"].view(np.uint32)) and np.array_equal(a["tri_index"], b["tri_index"])
                and np.array_equal(a["mesh_root"], b["mesh_root"]))


@pytest.mark.parametrize("variant", L.SAH_VARIANTS + L.RADIX_VARIANTS)
def test_negative_controls_change_a_tree_of_the_gpu_scenes(variant):
    """One decision changed — the exact comparison on the GPU test's scenes must be able to see it."""
    seen = []
    for name, fn in L.GPU_SCENES.items():
        if name == "c3_69600":
            continue
        sc = fn()
        for builder in (3,) if variant in L.SAH_VARIANTS else (1, 2):
            if differs(L.build(sc, builder, 2), L.build(sc, builder, 2, variant=variant)):
                seen.append((name, builder))
    print(variant, seen)
    assert seen, f"no scene of the GPU test shows variant {variant}"
    if variant in L.RADIX_VARIANTS:
        assert {b for _, b in seen} == {1, 2}


def test_full_size_restatement_is_fast_enough():
    """69,600 triangles through all three restated builders: recorded, with a generous ceiling so that the GPU test stays usable."""
    sc = L.GPU_SCENES["c3_69600"]()
    t0 = time.time()
    trees = [L.build(sc, b, 2) for b in (1, 2, 3)]
    dt = time.time() - t0
    print(f"restatement of builders 1, 2, 3 on {sc.n_triangles} triangles: {dt:.1f} s; nodes {[t['n_nodes'] for t in trees]}, depth {[t['max_depth'] for t in trees]}")
    assert trees[2]["n_halved"] == 0 and dt < 60.0
