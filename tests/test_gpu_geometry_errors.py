"""GPU: what the device-geometry entry points of include/urt.h answer to a wrong call — urt_skin_vertices, urt_buffer_bounds, the three
object-BVH calls, the normals and morph plans with urt_compute_normals / urt_morph_vertices, and the buffer arguments of
urt_reproject_deformed.  One literal table of (call, arguments, return code, urt_last_error text): every handle 0 and unknown, every wrong
stride and count, every input given as a destination, unknown and released plans, empty ranges after valid and invalid arguments.  A
text of None marks a call that is wrong in two ways: the code is pinned — it fixes which KIND of check comes first — the message may name
either fault.  The texts were recorded from the library as it was before these calls shared their argument checks, and the table has not
been edited since.  No wrong call changes a buffer's state or the deform counters, and a valid call of each kind succeeds afterwards."""
import ctypes as C

import numpy as np
import pytest

from unityraytracer_amd import ComputeBuffer, ComputeShader, Context, RenderTexture, _lib, scenes

pytestmark = pytest.mark.gpu

OK, ARGUMENT, HANDLE, SCENE = 0, 1, 2, 8
UNKNOWN = 0xdead
N = 40

# name -> (count, stride).  In a table entry a string names one of these buffers (or a plan, below), an int is passed as it is.
BUFFERS = {
    "rest_v": (N, 12), "rest_n": (N, 12), "dst_v": (N, 12), "dst_n": (N, 12), "verts": (N, 12), "spare12": (N, 12), "long12": (N + 1, 12),
    "idx": (N, 16), "wgt": (N, 16), "spare16": (N, 16), "long16": (N + 1, 16),
    "bones": (3, 48), "weights": (3, 4), "weights4": (4, 4),
    "indices": (6, 4), "indices4": (4, 4), "indices_far": (3, 4), "flags": (2, 4),
    "meshes": (2, 112), "meshes_far": (2, 112), "spheres": (2, 56),
    "leaves": (2, 28), "leaves_b": (2, 28), "nodes": (3, 28), "one28": (1, 28), "many28": (1025, 28),
}
# the plans: "nplan" serves verts[0..40) over `indices`, "nplan0" an empty range of it, "nplan_orphan" a vertices buffer released since;
# "mplan" serves [0, 40) with 3 targets, "mplan0" an empty range, "mplan_long" [0, 41); "released_*" were released
SKIN = dict(rest_v="rest_v", rest_n="rest_n", idx="idx", wgt="wgt", bones="bones", dst_v="dst_v", dst_n="dst_n", first=0, count=5)
MORPH = dict(plan="mplan", rest_v="rest_v", rest_n="rest_n", weights="weights", dst_v="dst_v", dst_n="dst_n", flags=0)
MESH_LEAF = dict(meshes="meshes", verts="verts", indices="indices", dst="leaves")
SPHERE_LEAF = dict(spheres="spheres", dst="leaves")
BUILD = dict(leaves="leaves", dst="nodes")
NPLAN = dict(verts="verts", indices="indices", first=0, count=N)
NORMALS = dict(plan="nplan", dst="dst_n")
DEFORM = dict(v="verts", i="indices", o="meshes", f="flags", table="bones", table2=0)
BOUNDS = dict(buffer="dst_v", first=0, count=5)

T = [
    # ---- urt_skin_vertices
    ("skin", dict(rest_v=0), HANDLE, "skin_vertices: rest_vertices is 0 or an unknown buffer handle"),
    ("skin", dict(rest_v=UNKNOWN), HANDLE, "skin_vertices: rest_vertices is 0 or an unknown buffer handle"),
    ("skin", dict(rest_n=UNKNOWN), HANDLE, "skin_vertices: rest_normals is 0 or an unknown buffer handle"),
    ("skin", dict(idx=0), HANDLE, "skin_vertices: bone_indices is 0 or an unknown buffer handle"),
    ("skin", dict(idx=UNKNOWN), HANDLE, "skin_vertices: bone_indices is 0 or an unknown buffer handle"),
    ("skin", dict(wgt=0), HANDLE, "skin_vertices: bone_weights is 0 or an unknown buffer handle"),
    ("skin", dict(wgt=UNKNOWN), HANDLE, "skin_vertices: bone_weights is 0 or an unknown buffer handle"),
    ("skin", dict(bones=0), HANDLE, "skin_vertices: bones is 0 or an unknown buffer handle"),
    ("skin", dict(bones=UNKNOWN), HANDLE, "skin_vertices: bones is 0 or an unknown buffer handle"),
    ("skin", dict(dst_v=0), HANDLE, "skin_vertices: dst_vertices is 0 or an unknown buffer handle"),
    ("skin", dict(dst_v=UNKNOWN), HANDLE, "skin_vertices: dst_vertices is 0 or an unknown buffer handle"),
    ("skin", dict(dst_n=UNKNOWN), HANDLE, "skin_vertices: dst_normals is 0 or an unknown buffer handle"),
    ("skin", dict(dst_n=0, rest_n=UNKNOWN), HANDLE, "skin_vertices: rest_normals is an unknown buffer handle"),
    ("skin", dict(rest_n=0), ARGUMENT, "skin_vertices: dst_normals without rest_normals"),
    ("skin", dict(null_in=True), ARGUMENT, "skin_vertices: in is NULL"),
    ("skin", dict(rest_v="spare16"), ARGUMENT, "skin_vertices: the stride of rest_vertices is not 12"),
    ("skin", dict(rest_n="spare16"), ARGUMENT, "skin_vertices: the stride of rest_normals is not 12"),
    ("skin", dict(idx="spare12"), ARGUMENT, "skin_vertices: the stride of bone_indices is not 16"),
    ("skin", dict(wgt="spare12"), ARGUMENT, "skin_vertices: the stride of bone_weights is not 16"),
    ("skin", dict(bones="spare16"), ARGUMENT, "skin_vertices: the stride of bones is not 48"),
    ("skin", dict(dst_v="spare16"), ARGUMENT, "skin_vertices: the stride of dst_vertices is not 12"),
    ("skin", dict(dst_n="spare16"), ARGUMENT, "skin_vertices: the stride of dst_normals is not 12"),
    ("skin", dict(rest_v="long12"), ARGUMENT, "skin_vertices: the count of rest_normals is not that of rest_vertices"),
    ("skin", dict(rest_n="long12"), ARGUMENT, "skin_vertices: the count of rest_normals is not that of rest_vertices"),
    ("skin", dict(idx="long16"), ARGUMENT, "skin_vertices: the count of bone_indices is not that of rest_vertices"),
    ("skin", dict(wgt="long16"), ARGUMENT, "skin_vertices: the count of bone_weights is not that of rest_vertices"),
    ("skin", dict(dst_v="long12"), ARGUMENT, "skin_vertices: the count of dst_vertices is not that of rest_vertices"),
    ("skin", dict(dst_n="long12"), ARGUMENT, "skin_vertices: the count of dst_normals is not that of rest_vertices"),
    ("skin", dict(dst_v="rest_v"), ARGUMENT, "skin_vertices: rest_vertices is also a destination"),
    ("skin", dict(dst_v="rest_n"), ARGUMENT, "skin_vertices: rest_normals is also a destination"),
    ("skin", dict(dst_n="rest_v"), ARGUMENT, "skin_vertices: rest_vertices is also a destination"),
    ("skin", dict(dst_n="rest_n"), ARGUMENT, "skin_vertices: rest_normals is also a destination"),
    ("skin", dict(dst_n="dst_v"), ARGUMENT, "skin_vertices: dst_vertices and dst_normals are one buffer"),
    ("skin", dict(first=-1, count=1), ARGUMENT, "skin_vertices: the element range lies outside the buffer"),
    ("skin", dict(first=0, count=-1), ARGUMENT, "skin_vertices: the element range lies outside the buffer"),
    ("skin", dict(first=36, count=5), ARGUMENT, "skin_vertices: the element range lies outside the buffer"),
    ("skin", dict(first=2 ** 31 - 1, count=2), ARGUMENT, "skin_vertices: the element range lies outside the buffer"),
    ("skin", dict(count=0), OK, None),
    ("skin", dict(count=0, rest_n=0, dst_n=0), OK, None),
    ("skin", dict(count=0, dst_v="rest_v"), ARGUMENT, "skin_vertices: rest_vertices is also a destination"),
    ("skin", dict(count=0, bones=UNKNOWN), HANDLE, "skin_vertices: bones is 0 or an unknown buffer handle"),
    ("skin", dict(rest_n=0, rest_v=UNKNOWN), ARGUMENT, None),                     # dst_normals without rest_normals: before any lookup
    ("skin", dict(rest_v="spare16", dst_v=UNKNOWN), HANDLE, None),                # handles before strides,
    ("skin", dict(rest_n="long12", bones=UNKNOWN), HANDLE, None),                 # counts
    ("skin", dict(dst_v="rest_v", bones=0), HANDLE, None),                        # and aliasing
    ("skin", dict(dst_v="idx"), ARGUMENT, None),                                  # (an input of another stride as the destination)
    # ---- urt_buffer_bounds
    ("bounds", dict(buffer=0), HANDLE, "buffer_bounds: unknown buffer handle"),
    ("bounds", dict(buffer=UNKNOWN), HANDLE, "buffer_bounds: unknown buffer handle"),
    ("bounds", dict(buffer="idx"), ARGUMENT, "buffer_bounds: the stride of the buffer is not 12"),
    ("bounds", dict(first=36, count=5), ARGUMENT, "buffer_bounds: the element range lies outside the buffer"),
    ("bounds", dict(first=-1, count=1), ARGUMENT, "buffer_bounds: the element range lies outside the buffer"),
    ("bounds", dict(null_out=True), ARGUMENT, "buffer_bounds: out6 is NULL"),
    ("bounds", dict(buffer=UNKNOWN, null_out=True), HANDLE, None),
    # ---- urt_morph_vertices
    ("morph", dict(plan=0), HANDLE, "morph_vertices: unknown plan handle"),
    ("morph", dict(plan=UNKNOWN), HANDLE, "morph_vertices: unknown plan handle"),
    ("morph", dict(plan="released_mplan"), HANDLE, "morph_vertices: unknown plan handle"),
    ("morph", dict(plan="nplan"), HANDLE, "morph_vertices: unknown plan handle"),   # a plan of the other kind
    ("morph", dict(flags=2), ARGUMENT, "morph_vertices: unknown flags"),
    ("morph", dict(flags=1, rest_n=0, dst_n=0), ARGUMENT, "morph_vertices: URT_MORPH_NORMALIZE without dst_normals"),
    ("morph", dict(rest_n=0), ARGUMENT, "morph_vertices: dst_normals without rest_normals"),
    ("morph", dict(rest_v=0), HANDLE, "morph_vertices: rest_vertices is 0 or an unknown buffer handle"),
    ("morph", dict(rest_v=UNKNOWN), HANDLE, "morph_vertices: rest_vertices is 0 or an unknown buffer handle"),
    ("morph", dict(rest_n=UNKNOWN), HANDLE, "morph_vertices: rest_normals is 0 or an unknown buffer handle"),
    ("morph", dict(weights=0), HANDLE, "morph_vertices: weights is 0 or an unknown buffer handle"),
    ("morph", dict(weights=UNKNOWN), HANDLE, "morph_vertices: weights is 0 or an unknown buffer handle"),
    ("morph", dict(dst_v=0), HANDLE, "morph_vertices: dst_vertices is 0 or an unknown buffer handle"),
    ("morph", dict(dst_v=UNKNOWN), HANDLE, "morph_vertices: dst_vertices is 0 or an unknown buffer handle"),
    ("morph", dict(dst_n=UNKNOWN), HANDLE, "morph_vertices: dst_normals is 0 or an unknown buffer handle"),
    ("morph", dict(dst_n=0, rest_n=UNKNOWN), HANDLE, "morph_vertices: rest_normals is an unknown buffer handle"),
    ("morph", dict(rest_v="spare16"), ARGUMENT, "morph_vertices: the stride of rest_vertices is not 12"),
    ("morph", dict(rest_n="spare16"), ARGUMENT, "morph_vertices: the stride of rest_normals is not 12"),
    ("morph", dict(weights="bones"), ARGUMENT, "morph_vertices: the stride of weights is not 4"),
    ("morph", dict(dst_v="spare16"), ARGUMENT, "morph_vertices: the stride of dst_vertices is not 12"),
    ("morph", dict(dst_n="spare16"), ARGUMENT, "morph_vertices: the stride of dst_normals is not 12"),
    ("morph", dict(rest_v="long12"), ARGUMENT, "morph_vertices: the count of rest_normals is not that of rest_vertices"),
    ("morph", dict(rest_n="long12"), ARGUMENT, "morph_vertices: the count of rest_normals is not that of rest_vertices"),
    ("morph", dict(dst_v="long12"), ARGUMENT, "morph_vertices: the count of dst_vertices is not that of rest_vertices"),
    ("morph", dict(dst_n="long12"), ARGUMENT, "morph_vertices: the count of dst_normals is not that of rest_vertices"),
    ("morph", dict(weights="weights4"), ARGUMENT, "morph_vertices: the count of weights is not the plan's n_targets"),
    ("morph", dict(dst_v="rest_v"), ARGUMENT, "morph_vertices: rest_vertices is also a destination"),
    ("morph", dict(dst_n="rest_n"), ARGUMENT, "morph_vertices: rest_normals is also a destination"),
    ("morph", dict(dst_n="rest_v"), ARGUMENT, "morph_vertices: rest_vertices is also a destination"),
    ("morph", dict(dst_n="dst_v"), ARGUMENT, "morph_vertices: dst_vertices and dst_normals are one buffer"),
    ("morph", dict(plan="mplan_long"), ARGUMENT, "morph_vertices: the element range lies outside the buffer"),
    ("morph", dict(plan="mplan0"), OK, None),
    ("morph", dict(plan="mplan0", rest_n=0, dst_n=0), OK, None),
    ("morph", dict(plan="mplan0", dst_v="rest_v"), ARGUMENT, "morph_vertices: rest_vertices is also a destination"),
    ("morph", dict(plan="mplan0", weights=UNKNOWN), HANDLE, "morph_vertices: weights is 0 or an unknown buffer handle"),
    ("morph", dict(plan=UNKNOWN, flags=2), HANDLE, None),                         # the plan before the flags,
    ("morph", dict(flags=2, rest_v=UNKNOWN), ARGUMENT, None),                     # the flags before any lookup,
    ("morph", dict(rest_n=0, weights=UNKNOWN), ARGUMENT, None),                   # as dst_normals without rest_normals;
    ("morph", dict(rest_v="spare16", dst_v=UNKNOWN), HANDLE, None),               # handles before strides, counts and aliasing
    ("morph", dict(weights="weights4", dst_n=UNKNOWN), HANDLE, None),
    ("morph", dict(dst_v="rest_v", dst_n=UNKNOWN), HANDLE, None),
    # ---- urt_mesh_leaf_bounds_device
    ("mesh_leaf", dict(meshes=0), HANDLE, "mesh_leaf_bounds_device: mesh_objects is 0 or an unknown buffer handle"),
    ("mesh_leaf", dict(meshes=UNKNOWN), HANDLE, "mesh_leaf_bounds_device: mesh_objects is 0 or an unknown buffer handle"),
    ("mesh_leaf", dict(verts=0), HANDLE, "mesh_leaf_bounds_device: vertices is 0 or an unknown buffer handle"),
    ("mesh_leaf", dict(verts=UNKNOWN), HANDLE, "mesh_leaf_bounds_device: vertices is 0 or an unknown buffer handle"),
    ("mesh_leaf", dict(indices=0), HANDLE, "mesh_leaf_bounds_device: indices is 0 or an unknown buffer handle"),
    ("mesh_leaf", dict(indices=UNKNOWN), HANDLE, "mesh_leaf_bounds_device: indices is 0 or an unknown buffer handle"),
    ("mesh_leaf", dict(dst=0), HANDLE, "mesh_leaf_bounds_device: dst_leaves is 0 or an unknown buffer handle"),
    ("mesh_leaf", dict(dst=UNKNOWN), HANDLE, "mesh_leaf_bounds_device: dst_leaves is 0 or an unknown buffer handle"),
    ("mesh_leaf", dict(meshes="spheres"), ARGUMENT, "mesh_leaf_bounds_device: the stride of mesh_objects is not 112"),
    ("mesh_leaf", dict(verts="spare16"), ARGUMENT, "mesh_leaf_bounds_device: the stride of vertices is not 12"),
    ("mesh_leaf", dict(indices="spare12"), ARGUMENT, "mesh_leaf_bounds_device: the stride of indices is not 4"),
    ("mesh_leaf", dict(dst="spheres"), ARGUMENT, "mesh_leaf_bounds_device: the stride of dst_leaves is not 28"),
    ("mesh_leaf", dict(dst="nodes"), ARGUMENT, "mesh_leaf_bounds_device: the count of dst_leaves is not that of mesh_objects"),
    ("mesh_leaf", dict(meshes="meshes_far"), SCENE, "mesh_leaf_bounds_device: MeshObject 1 names a range outside indices"),
    ("mesh_leaf", dict(dst="meshes"), ARGUMENT, None),                            # (an input as the destination has the wrong stride too)
    ("mesh_leaf", dict(dst="indices"), ARGUMENT, None),
    ("mesh_leaf", dict(meshes="spheres", dst=UNKNOWN), HANDLE, None),
    ("mesh_leaf", dict(dst="nodes", verts=0), HANDLE, None),
    ("mesh_leaf", dict(meshes="meshes_far", dst="nodes"), ARGUMENT, None),        # the arguments before the contents
    # ---- urt_sphere_leaf_bounds_device
    ("sphere_leaf", dict(spheres=0), HANDLE, "sphere_leaf_bounds_device: spheres is 0 or an unknown buffer handle"),
    ("sphere_leaf", dict(spheres=UNKNOWN), HANDLE, "sphere_leaf_bounds_device: spheres is 0 or an unknown buffer handle"),
    ("sphere_leaf", dict(dst=0), HANDLE, "sphere_leaf_bounds_device: dst_leaves is 0 or an unknown buffer handle"),
    ("sphere_leaf", dict(dst=UNKNOWN), HANDLE, "sphere_leaf_bounds_device: dst_leaves is 0 or an unknown buffer handle"),
    ("sphere_leaf", dict(spheres="meshes"), ARGUMENT, "sphere_leaf_bounds_device: the stride of spheres is not 56"),
    ("sphere_leaf", dict(dst="meshes"), ARGUMENT, "sphere_leaf_bounds_device: the stride of dst_leaves is not 28"),
    ("sphere_leaf", dict(dst="nodes"), ARGUMENT, "sphere_leaf_bounds_device: the count of dst_leaves is not that of spheres"),
    ("sphere_leaf", dict(dst="spheres"), ARGUMENT, None),
    ("sphere_leaf", dict(spheres="meshes", dst=0), HANDLE, None),
    # ---- urt_build_object_bvh_device
    ("build", dict(leaves=0), HANDLE, "build_object_bvh_device: leaves is 0 or an unknown buffer handle"),
    ("build", dict(leaves=UNKNOWN), HANDLE, "build_object_bvh_device: leaves is 0 or an unknown buffer handle"),
    ("build", dict(dst=0), HANDLE, "build_object_bvh_device: dst_nodes is 0 or an unknown buffer handle"),
    ("build", dict(dst=UNKNOWN), HANDLE, "build_object_bvh_device: dst_nodes is 0 or an unknown buffer handle"),
    ("build", dict(leaves="spheres"), ARGUMENT, "build_object_bvh_device: the stride of leaves is not 28"),
    ("build", dict(dst="bones"), ARGUMENT, "build_object_bvh_device: the stride of dst_nodes is not 28"),
    ("build", dict(dst="leaves_b"), ARGUMENT, "build_object_bvh_device: the count of dst_nodes is not urt_host_object_bvh_length(2) = 3"),
    ("build", dict(leaves="many28"), ARGUMENT, "build_object_bvh_device: more than 1024 leaves: build this heap with urt_host_build_object_bvh"),   # (the limit comes before the count of dst_nodes)
    ("build", dict(leaves="one28", dst="one28"), ARGUMENT, "build_object_bvh_device: leaves is also the destination"),
    ("build", dict(leaves="nodes", dst="nodes"), ARGUMENT, None),                 # (... and 3 leaves want 7 nodes)
    ("build", dict(leaves="spheres", dst=UNKNOWN), HANDLE, None),
    # ---- urt_normals_plan_create / _info / _release, urt_compute_normals
    ("nplan", dict(verts=0), HANDLE, "normals_plan_create: vertices is 0 or an unknown buffer handle"),
    ("nplan", dict(verts=UNKNOWN), HANDLE, "normals_plan_create: vertices is 0 or an unknown buffer handle"),
    ("nplan", dict(indices=0), HANDLE, "normals_plan_create: indices is 0 or an unknown buffer handle"),
    ("nplan", dict(indices=UNKNOWN), HANDLE, "normals_plan_create: indices is 0 or an unknown buffer handle"),
    ("nplan", dict(verts="spare16"), ARGUMENT, "normals_plan_create: the stride of vertices is not 12"),
    ("nplan", dict(indices="spare12"), ARGUMENT, "normals_plan_create: the stride of indices is not 4"),
    ("nplan", dict(indices="indices4"), ARGUMENT, "normals_plan_create: the count of indices is not a multiple of 3"),
    ("nplan", dict(first=36, count=5), ARGUMENT, "normals_plan_create: the element range lies outside the buffer"),
    ("nplan", dict(first=-1, count=1), ARGUMENT, "normals_plan_create: the element range lies outside the buffer"),
    ("nplan", dict(indices="indices_far"), SCENE, "normals_plan_create: index outside _Vertices"),
    ("nplan", dict(null_out=True), ARGUMENT, "normals_plan_create: out_plan is NULL"),
    ("nplan", dict(verts="spare16", indices=UNKNOWN), HANDLE, None),
    ("nplan", dict(first=36, count=5, verts=0), HANDLE, None),
    ("nplan_info", dict(plan=0), HANDLE, "normals_plan_info: unknown plan handle"),
    ("nplan_info", dict(plan="released_nplan"), HANDLE, "normals_plan_info: unknown plan handle"),
    ("nplan_info", dict(plan="mplan"), HANDLE, "normals_plan_info: unknown plan handle"),
    ("nplan_info", dict(plan="nplan", null_out=True), ARGUMENT, "normals_plan_info: out is NULL"),
    ("nplan_release", dict(plan=UNKNOWN), HANDLE, "normals_plan_release: unknown plan handle"),
    ("nplan_release", dict(plan="released_nplan"), HANDLE, "normals_plan_release: unknown plan handle"),
    ("normals", dict(plan=0), HANDLE, "compute_normals: unknown plan handle"),
    ("normals", dict(plan=UNKNOWN), HANDLE, "compute_normals: unknown plan handle"),
    ("normals", dict(plan="released_nplan"), HANDLE, "compute_normals: unknown plan handle"),
    ("normals", dict(plan="nplan_orphan"), HANDLE, "compute_normals: the plan's vertices buffer was released"),
    ("normals", dict(dst=0), HANDLE, "compute_normals: dst_normals is 0 or an unknown buffer handle"),
    ("normals", dict(dst=UNKNOWN), HANDLE, "compute_normals: dst_normals is 0 or an unknown buffer handle"),
    ("normals", dict(dst="spare16"), ARGUMENT, "compute_normals: the stride of dst_normals is not 12"),
    ("normals", dict(dst="long12"), ARGUMENT, "compute_normals: the count of dst_normals is not that of the vertices buffer"),
    ("normals", dict(dst="verts"), ARGUMENT, "compute_normals: dst_normals is the vertices buffer"),
    ("normals", dict(plan="nplan0"), OK, None),
    ("normals", dict(plan="nplan0", dst="verts"), ARGUMENT, "compute_normals: dst_normals is the vertices buffer"),
    ("normals", dict(plan="nplan0", dst=UNKNOWN), HANDLE, "compute_normals: dst_normals is 0 or an unknown buffer handle"),
    ("normals", dict(plan=UNKNOWN, dst="spare16"), HANDLE, None),
    # ---- urt_morph_plan_create / _info / _release
    ("mplan", dict(n_deltas=-1), ARGUMENT, "morph_plan_create: a negative n_deltas, first or count, or a served range beyond 2^31 - 1"),
    ("mplan", dict(first=2 ** 31 - 1, count=1), ARGUMENT, "morph_plan_create: a negative n_deltas, first or count, or a served range beyond 2^31 - 1"),
    ("mplan", dict(null_deltas=True), ARGUMENT, "morph_plan_create: deltas is NULL"),
    ("mplan", dict(n_targets=0), ARGUMENT, "morph_plan_create: n_targets is outside 1..4096"),
    ("mplan", dict(n_targets=4097), ARGUMENT, "morph_plan_create: n_targets is outside 1..4096"),
    ("mplan", dict(first=1), SCENE, "morph_plan_create: a delta names a vertex outside the served range"),
    ("mplan", dict(n_targets=2), SCENE, "morph_plan_create: a delta names a target outside 0..n_targets-1"),
    ("mplan", dict(null_out=True), ARGUMENT, "morph_plan_create: out_plan is NULL"),
    ("mplan_info", dict(plan=0), HANDLE, "morph_plan_info: unknown plan handle"),
    ("mplan_info", dict(plan="released_mplan"), HANDLE, "morph_plan_info: unknown plan handle"),
    ("mplan_info", dict(plan="nplan"), HANDLE, "morph_plan_info: unknown plan handle"),
    ("mplan_info", dict(plan="mplan", null_out=True), ARGUMENT, "morph_plan_info: out is NULL"),
    ("mplan_release", dict(plan=UNKNOWN), HANDLE, "morph_plan_release: unknown plan handle"),
    ("mplan_release", dict(plan="released_mplan"), HANDLE, "morph_plan_release: unknown plan handle"),
    # ---- urt_reproject_deformed: the four buffers of urt_ReprojectDeform and the two motion tables
    ("deform", dict(v=0), HANDLE, "reproject: prev_vertices is 0 or an unknown buffer handle"),
    ("deform", dict(v=UNKNOWN), HANDLE, "reproject: prev_vertices is 0 or an unknown buffer handle"),
    ("deform", dict(i=0), HANDLE, "reproject: indices is 0 or an unknown buffer handle"),
    ("deform", dict(i=UNKNOWN), HANDLE, "reproject: indices is 0 or an unknown buffer handle"),
    ("deform", dict(o=0), HANDLE, "reproject: prev_mesh_objects is 0 or an unknown buffer handle"),
    ("deform", dict(o=UNKNOWN), HANDLE, "reproject: prev_mesh_objects is 0 or an unknown buffer handle"),
    ("deform", dict(f=0), HANDLE, "reproject: deformed is 0 or an unknown buffer handle"),
    ("deform", dict(f=UNKNOWN), HANDLE, "reproject: deformed is 0 or an unknown buffer handle"),
    ("deform", dict(v="spare16"), ARGUMENT, "reproject: the stride of prev_vertices is not 12"),
    ("deform", dict(i="spare12"), ARGUMENT, "reproject: the stride of indices is not 4"),
    ("deform", dict(o="spheres"), ARGUMENT, "reproject: the stride of prev_mesh_objects is not 112"),
    ("deform", dict(f="spheres"), ARGUMENT, "reproject: the stride of deformed is not 4"),
    ("deform", dict(i="indices4"), ARGUMENT, "reproject: the count of indices is not a multiple of 3"),
    ("deform", dict(f="weights"), ARGUMENT, "reproject: the counts of deformed and prev_mesh_objects differ"),
    ("deform", dict(table=UNKNOWN), HANDLE, "reproject: unknown mesh_motion buffer handle"),
    ("deform", dict(table2=UNKNOWN), HANDLE, "reproject: unknown sphere_motion buffer handle"),
    ("deform", dict(table="spare16"), ARGUMENT, "reproject: the stride of mesh_motion is not 48"),
    ("deform", dict(table2="spare16"), ARGUMENT, "reproject: the stride of sphere_motion is not 48"),
    ("deform", dict(v="spare16", i=UNKNOWN), ARGUMENT, None),                     # here each buffer is looked up and measured in turn
    ("deform", dict(v=UNKNOWN, i="spare12"), HANDLE, None),
    ("deform", dict(table="spare16", v=UNKNOWN), ARGUMENT, None),                 # ... the motion tables first
    ("deform", dict(i="indices4", f=UNKNOWN), HANDLE, None),
]


def test_every_wrong_call_answers_as_recorded_and_changes_nothing(gpu_ctx):
    w, h = 16, 8
    with Context(gpu_ctx.device) as ctx:
        lib, hd = ctx.lib, ctx._h
        rng = np.random.default_rng(11)
        B = {name: ComputeBuffer(ctx, count, stride) for name, (count, stride) in BUFFERS.items()}
        for name in ("rest_v", "rest_n", "verts"):
            B[name].SetData(rng.uniform(-1, 1, (N, 3)).astype(np.float32))
        B["idx"].SetData(rng.integers(0, 3, (N, 4)).astype(np.int32))
        B["wgt"].SetData(np.full((N, 4), 0.25, np.float32))
        B["bones"].SetData(np.tile(np.eye(4, dtype=np.float32)[:3].reshape(12), (3, 1)))
        B["weights"].SetData(np.array([0.5, 0.25, 0.0], np.float32))
        B["indices"].SetData(np.array([0, 1, 2, 3, 4, 5], np.int32))
        B["indices_far"].SetData(np.array([0, 1, N], np.int32))
        for name, ranges in (("meshes", ((0, 3), (3, 3))), ("meshes_far", ((0, 3), (3, 4)))):
            mo = np.zeros(2, scenes.MESHOBJECT_DT)
            mo["localToWorldMatrix"] = np.eye(4, dtype=np.float32).reshape(16)
            mo["indices_offset"], mo["indices_count"] = zip(*ranges)
            B[name].SetData(mo)
        sp = np.zeros(2, scenes.SPHERE_DT)
        sp["radius"] = 1
        B["spheres"].SetData(sp)
        B["flags"].SetData(np.array([1, 0], np.int32))
        names = ("prev_color", "prev_count", "prev_hit", "prev_normal", "prev_id", "hit", "normal", "id", "color", "count", "motion")
        tex = [RenderTexture(ctx, w, h) for _ in names]
        images = C.byref(_lib.ReprojectImages(*(t.handle for t in tex)))
        params = C.byref(_lib.ReprojectParams((C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16).tolist()), 64.0, 0.9, 0.02, 0))
        sh = ComputeShader(ctx)
        sh.SetMatrix("_CameraToWorld", scenes.camera_matrices(w, h)[0])
        sh.SetMatrix("_CameraInverseProjection", scenes.camera_matrices(w, h)[1])
        deltas = np.zeros(3, _lib.MORPH_DELTA_DT)
        deltas["vertex"], deltas["target"], deltas["dp"] = (0, 5, N - 1), (0, 1, 2), 0.5

        def handle(v):
            return B[v].handle if v in B else P[v] if isinstance(v, str) else v

        def skin(a):
            sb = _lib.SkinBuffers(*(handle(a[k]) for k in ("rest_v", "rest_n", "idx", "wgt", "bones")))
            return lib.urt_skin_vertices(hd, None if a.get("null_in") else C.byref(sb), a["first"], a["count"], handle(a["dst_v"]), handle(a["dst_n"]))

        def bounds(a):
            return lib.urt_buffer_bounds(hd, handle(a["buffer"]), a["first"], a["count"], None if a.get("null_out") else (C.c_float * 6)(), None)

        def morph(a):
            return lib.urt_morph_vertices(hd, *(handle(a[k]) for k in ("plan", "rest_v", "rest_n", "weights", "dst_v", "dst_n")), a["flags"])

        def new_plan(create, *args, null_out=False):
            """(code, handle): a failed creation must have zeroed *out_plan."""
            out = C.c_uint64(77)
            rc = create(hd, *args, None if null_out else C.byref(out))
            assert null_out or (out.value == 0) == (rc != 0)
            return rc, out.value

        def nplan(a):
            return new_plan(lib.urt_normals_plan_create, handle(a["verts"]), handle(a["indices"]), a["first"], a["count"], null_out=a.get("null_out", False))

        def mplan(a):
            d = None if a.get("null_deltas") else deltas.ctypes.data_as(C.c_void_p)
            return new_plan(lib.urt_morph_plan_create, d, a.get("n_deltas", len(deltas)), a.get("n_targets", 3), a.get("first", 0), a.get("count", N),
                            null_out=a.get("null_out", False))

        def deform(a):
            mo = C.byref(_lib.ReprojectMotion(handle(a["table"]), handle(a["table2"]), 0.0, 0))
            de = C.byref(_lib.ReprojectDeform(handle(a["v"]), handle(a["i"]), handle(a["o"]), handle(a["f"]), 0.5, 0))
            return lib.urt_reproject_deformed(hd, images, params, mo, de)

        calls = {
            "skin": (SKIN, skin), "bounds": (BOUNDS, bounds), "morph": (MORPH, morph), "deform": (DEFORM, deform),
            "mesh_leaf": (MESH_LEAF, lambda a: lib.urt_mesh_leaf_bounds_device(hd, *(handle(a[k]) for k in ("meshes", "verts", "indices", "dst")))),
            "sphere_leaf": (SPHERE_LEAF, lambda a: lib.urt_sphere_leaf_bounds_device(hd, handle(a["spheres"]), handle(a["dst"]))),
            "build": (BUILD, lambda a: lib.urt_build_object_bvh_device(hd, handle(a["leaves"]), handle(a["dst"]))),
            "nplan": (NPLAN, lambda a: nplan(a)[0]), "mplan": ({}, lambda a: mplan(a)[0]),
            "normals": (NORMALS, lambda a: lib.urt_compute_normals(hd, handle(a["plan"]), handle(a["dst"]))),
            "nplan_info": ({}, lambda a: lib.urt_normals_plan_info(hd, handle(a["plan"]), None if a.get("null_out") else C.byref(_lib.NormalsPlanInfo()))),
            "mplan_info": ({}, lambda a: lib.urt_morph_plan_info(hd, handle(a["plan"]), None if a.get("null_out") else C.byref(_lib.MorphPlanInfo()))),
            "nplan_release": ({}, lambda a: lib.urt_normals_plan_release(hd, handle(a["plan"]))),
            "mplan_release": ({}, lambda a: lib.urt_morph_plan_release(hd, handle(a["plan"]))),
        }

        # the plans of the table
        P = {}
        orphan = ComputeBuffer(ctx, N, 12)
        for name, (rc, plan) in {"nplan": nplan(NPLAN), "nplan0": nplan(dict(NPLAN, count=0)), "released_nplan": nplan(NPLAN),
                                 "nplan_orphan": nplan(dict(NPLAN, verts=orphan.handle)),
                                 "mplan": mplan({}), "mplan0": mplan(dict(n_deltas=0, null_deltas=True, count=0)),
                                 "mplan_long": mplan(dict(count=N + 1)), "released_mplan": mplan({})}.items():
            assert rc == OK and plan != 0, (name, rc, lib.urt_last_error(hd))
            P[name] = plan
        orphan.Release()
        assert lib.urt_normals_plan_release(hd, P["released_nplan"]) == OK and lib.urt_morph_plan_release(hd, P["released_mplan"]) == OK

        assert skin(dict(SKIN, first=2, count=10)) == OK                              # (a mirror and a stale range to keep)
        before = {name: ctx.buffer_state(b) for name, b in B.items()}
        stats = ctx.deform_stats()
        assert before["dst_v"]["mirror_bytes"] == N * 12 and (before["dst_v"]["stale_first"], before["dst_v"]["stale_last"]) == (2, 11)
        assert before["verts"]["mirror_bytes"] == 0

        wrong = []
        for k, (call, over, code, text) in enumerate(T):
            base, fn = calls[call]
            assert set(over) <= set(base) | {"null_in", "null_out", "null_deltas", "n_deltas", "n_targets", "first", "count", "plan"}, (k, call, over)
            rc = fn(dict(base, **over))
            got = lib.urt_last_error(hd).decode()
            print(f"{k:3d} {call:13s} {over!r:60s} -> {rc} {got if rc else ''}")
            if rc != code or (text is not None and got != text):
                wrong.append((k, call, over, rc, got))
        assert not wrong, wrong
        assert {name: ctx.buffer_state(b) for name, b in B.items()} == before and ctx.deform_stats() == stats

        # a valid call of each kind still succeeds
        for call, over in (("skin", {}), ("skin", dict(rest_n=0, dst_n=0)), ("skin", dict(rest_n="rest_n", dst_n=0)), ("bounds", {}),
                           ("morph", {}), ("morph", dict(flags=1)), ("morph", dict(rest_n=0, dst_n=0)),
                           ("mesh_leaf", {}), ("sphere_leaf", dict(dst="leaves_b")), ("build", {}), ("normals", {}), ("deform", {}), ("deform", dict(table=0)),
                           ("nplan_info", dict(plan="nplan")), ("mplan_info", dict(plan="mplan"))):
            base, fn = calls[call]
            assert fn(dict(base, **over)) == OK, (call, over, lib.urt_last_error(hd))
        ctx.synchronize()
        after = {name: ctx.buffer_state(b) for name, b in B.items()}
        assert (after["dst_v"]["stale_first"], after["dst_v"]["stale_last"]) == (0, N - 1) and after["nodes"]["mirror_bytes"] == 3 * 28
        assert (after["leaves"]["stale_first"], after["leaves"]["stale_last"]) == (0, 1) and after["verts"]["mirror_bytes"] == N * 12
        for name in ("nplan", "nplan0", "nplan_orphan"):
            assert lib.urt_normals_plan_release(hd, P[name]) == OK
        for name in ("mplan", "mplan0", "mplan_long"):
            assert lib.urt_morph_plan_release(hd, P[name]) == OK
        for x in list(B.values()) + tex:
            x.Release()
