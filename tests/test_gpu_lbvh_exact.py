"""GPU: the trees of the three GPU triangle-BVH builders (csrc/lbvh.hip, blas_builder 1, 2, 3) ARE the trees of their numpy restatement
(tests/lbvh_ref.py, itself checked against the host builder and in float64 by tests/test_lbvh_ref.py): every word of every node, the
leaf order, the roots, the node count and the depth, bit for bit and without a tolerance.  Pixels cannot show this (any conservative
BVH gives the same frame); a sweep that takes the last minimum, a lost atomic in the LDS path, an unstable partition, a wrong Morton
cell or a box that is too large all change a tree and nothing else.  The builders are deterministic functions of the scene buffers
(integer atomics on order-preserving images of floats, a stable sort, no float reduction whose order matters), so equality is exact."""
import numpy as np
import pytest

import lbvh_ref as L
from unityraytracer_amd import RayTraceMaster

pytestmark = pytest.mark.gpu
NAMES = {1: "karras", 2: "budget", 3: "sah"}


@pytest.fixture
def ctx(gpu_ctx):
    gpu_ctx.set_option("kernel_mode", 3)
    try:
        yield gpu_ctx
    finally:
        gpu_ctx.set_option("blas_builder", -1)
        gpu_ctx.set_option("blas_leaf_max", 2)
        gpu_ctx.set_option("lbvh_slack", 6)


def device_tree(ctx, sc, builder, leaf_max=2, slack=6):
    """Binds the scene, renders one small frame (which prepares it) and reads the triangle BVH back."""
    ctx.set_option("blas_builder", builder)
    ctx.set_option("lbvh_slack", slack)
    ctx.set_option("blas_leaf_max", leaf_max)          # (always marks the scene stale: the next frame builds it again)
    m = RayTraceMaster(ctx, sc)
    try:
        m.OnRenderImage()
        assert ctx.launch_info()["blas_builder"] == builder
        nodes, tri, root, info = ctx.read_scene_blas(len(sc.mesh_objects))
    finally:
        m.OnDisable()
    return nodes, tri, root, info


def assert_is_the_restated_tree(got, ref, label):
    nodes, tri, root, info = got
    why = L.describe_mismatch(nodes, ref["nodes"], ref["level"])
    assert not why, f"{label}: {why}"
    assert np.array_equal(nodes.view(np.uint32), ref["nodes"].view(np.uint32)), label      # all 16 words, the two zero words included
    bad = np.nonzero(tri != ref["tri_index"])[0] if len(tri) == len(ref["tri_index"]) else [-1]
    assert len(bad) == 0, f"{label}: leaf order differs first at position {int(bad[0])} ({len(bad)} positions)"
    assert np.array_equal(root, ref["mesh_root"]), f"{label}: mesh_root {root.tolist()[:12]} against {ref['mesh_root'].tolist()[:12]}"
    assert info["n_nodes"] == ref["n_nodes"] and info["max_depth"] == ref["max_depth"], (label, info, ref["n_nodes"], ref["max_depth"])


@pytest.mark.parametrize("builder", [1, 2, 3], ids=NAMES.values())
@pytest.mark.parametrize("name", list(L.GPU_SCENES))
def test_device_tree_is_the_restated_tree(ctx, name, builder):
    sc = L.GPU_SCENES[name]()
    assert_is_the_restated_tree(device_tree(ctx, sc, builder), L.build(sc, builder, 2), f"{name}, builder {builder}")


@pytest.mark.parametrize("builder", [1, 2, 3], ids=NAMES.values())
@pytest.mark.parametrize("leaf_max", [1, 2, 4, 8])
@pytest.mark.parametrize("name", ["mixed", "thresholds", "degenerate"])
def test_every_leaf_size(ctx, name, leaf_max, builder):
    sc = L.GPU_SCENES[name]()
    assert_is_the_restated_tree(device_tree(ctx, sc, builder, leaf_max), L.build(sc, builder, leaf_max), f"{name}, builder {builder}, leaf_max {leaf_max}")


@pytest.mark.parametrize("slack", [0, 6])
@pytest.mark.parametrize("name", ["c3_5520", "thresholds", "degenerate", "deep_chain"])
def test_depth_budget_with_and_without_slack(ctx, name, slack):
    sc = L.GPU_SCENES[name]()
    ref = L.build(sc, 2, 2, slack)
    assert ref["max_depth"] <= ref["depth_cap"]
    assert_is_the_restated_tree(device_tree(ctx, sc, 2, 2, slack), ref, f"{name}, builder 2, slack {slack}")


@pytest.mark.parametrize("builder", [1, 2, 3], ids=NAMES.values())
def test_the_same_scene_prepared_twice_gives_the_same_bytes(ctx, builder):
    """Builder 2's queue order varies from run to run, the atomics of builder 3 arrive in any order: the tree must not."""
    sc = L.GPU_SCENES["c3_5520"]()
    a = device_tree(ctx, sc, builder)
    b = device_tree(ctx, sc, builder)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3]["max_depth"] == b[3]["max_depth"]


@pytest.mark.parametrize("builder", [1, 2, 3], ids=NAMES.values())
def test_non_finite_vertices_land_where_the_restatement_says(ctx, builder):
    """One mesh with a +inf, a -inf and a NaN vertex: the centroid bounds are infinite, cells and bins come out NaN or out of range, and
    the conversions the restatement defines (NaN -> 0, saturating) decide.  Built and read back only."""
    sc = L.nonfinite_scene()
    with np.errstate(all="ignore"):
        ref = L.build(sc, builder, 2)
    assert_is_the_restated_tree(device_tree(ctx, sc, builder), ref, f"non-finite, builder {builder}")
