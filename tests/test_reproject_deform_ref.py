"""CPU: the restatement of urt_reproject_deformed (tests/reproject_deform_ref.py) against the restatement of urt_reproject_objects and
against geometry: the two equivalences, a rigid move written as a vertex edit, unchanged vertices, the dead cases, and the conditions the
quality move of tests/test_gpu_reproject_deform.py must meet.  Feature buffers come from the brute-force caster of the same module."""
import numpy as np
import pytest

import reproject_deform_cases as K
from reproject_deform_ref import (QUALITY_BLOB, QUALITY_CAMERA, QUALITY_MESH, QUALITY_MIN_COVERAGE, QUALITY_MIN_KEPT, QUALITY_PHASE, QUALITY_SIZE,
                                  cast_aovs, matrices_of, reproject_deformed_ref)
from reproject_motion_ref import reproject_objects_ref
from unityraytracer_amd import scenes

F = np.float32


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b, keys=("color", "count", "motion")):
    return all(u32(a[k]).tobytes() == u32(b[k]).tobytes() for k in keys)


# ---- 1. the two equivalences -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(K.SETTINGS)))
def test_no_deform_and_zero_flags_equal_reproject_objects_bit_for_bit(k):
    images, mats, params, _ = K.settings_case(k, 40 + k, 67, 33)
    deform = params.pop("deform")
    objects = reproject_objects_ref(*images, *mats, **params)
    assert same_bits(reproject_deformed_ref(*images, *mats, deform=None, **params), objects)
    zero = (deform[0], deform[1], deform[2], np.zeros_like(deform[3]), deform[4])
    got = reproject_deformed_ref(*images, *mats, deform=zero, **params)
    assert not got["deformed"].any()
    o, kind = images[7].view(np.int32)[..., 0], images[6][..., 3]
    inside = ~((kind == 3) & ((o < 0) | (o >= len(deform[3]))))                  # a triangle pixel outside the tables has no history by definition
    for key in ("color", "count", "motion"):
        assert u32(got[key])[inside].tobytes() == u32(objects[key])[inside].tobytes(), key
    assert inside.mean() > 0.7
    flagged = reproject_deformed_ref(*images, *mats, deform=deform, **params)
    if k != 4:                                                                  # (the case with one object flags little)
        assert flagged["deformed"].any() and not same_bits(flagged, objects)


# ---- the mixed scene, cast on the CPU ------------------------------------------------------------------------------------------------------
SIZE = (96, 64)
NEAR = (-1.0, 1.5, -4.0)


def cast(sc, vertices=None, mesh_objects=None, size=SIZE, cam=None):
    cam = cam or (sc.camera_to_world, sc.camera_inverse_projection)
    return cast_aovs(*size, *cam, sc.mesh_objects if mesh_objects is None else mesh_objects, sc.vertices if vertices is None else vertices,
                     sc.indices, sc.normals, sc.spheres)


@pytest.fixture(scope="module")
def mixed():
    sc = scenes.mixed_test_scene(*SIZE)
    sc.camera_to_world, sc.camera_inverse_projection = scenes.camera_matrices(*SIZE, position=NEAR)   # the default camera sees the blob 8 pixels tall
    return sc, cast(sc)


def history(shape, seed=3):
    rng = np.random.default_rng(seed)
    color = rng.uniform(0.1, 2.0, shape + (4,)).astype(F)
    count = np.zeros(shape + (4,), F)
    count[..., 0] = rng.choice([1.0, 7.0, 40.0], shape)
    return color, count


def flags_for(sc, *meshes):
    f = np.zeros(len(sc.mesh_objects), np.int32)
    f[list(meshes)] = 1
    return f


def blob_span(sc):
    mo = sc.mesh_objects[0]
    sl = np.asarray(sc.indices[int(mo["indices_offset"]): int(mo["indices_offset"]) + int(mo["indices_count"])])
    return int(sl.min()), int(sl.max())


# ---- 2. a rigid move written as a vertex edit -----------------------------------------------------------------------------------------------
def test_rigid_move_through_the_vertices_agrees_with_the_motion_table(mixed):
    sc, prev = mixed
    lo, hi = blob_span(sc)
    a = np.radians(5.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    step = np.array([0.06, 0.02, -0.04])
    new_v = np.array(sc.vertices, np.float64)
    new_v[lo: hi + 1] = new_v[lo: hi + 1] @ R.T + step                          # object space: the blob turns about its own origin and shifts
    new_v = new_v.astype(F)
    cur = cast(sc, vertices=new_v)
    # the same move as a matrix: M_new = M * [R | step]; the table takes current world points to previous ones: M * inv(M_new)
    M = np.asarray(sc.mesh_objects[0]["localToWorldMatrix"], np.float64).reshape(4, 4).T
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, step
    back = M @ np.linalg.inv(M @ E)
    table = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F), (len(sc.mesh_objects), 1))
    table[0] = np.concatenate([back[:3, :3].T.reshape(9), back[:3, 3]]).astype(F)
    color, count = history(prev[0].shape[:2])
    Mx = scenes.world_to_clip(sc.camera_to_world, sc.camera_inverse_projection)
    cams = (Mx, sc.camera_to_world, sc.camera_inverse_projection)
    # the face normal against the shading normals of a 12 x 9 blob: the normal tests are taken out of the comparison on both sides
    by_table = reproject_objects_ref(color, count, *prev, *cur, *cams, mesh_motion=table, normal_threshold=-1.0)
    by_vertex = reproject_deformed_ref(color, count, *prev, *cur, *cams, normal_threshold=-1.0,
                                       deform=(sc.vertices, sc.indices, matrices_of(sc.mesh_objects), flags_for(sc, 0), -1.0))
    on = (cur[2].view(np.int32)[..., 0] == 0) & (cur[1][..., 3] == 3)
    assert on.mean() > 0.02 and (by_vertex["deformed"] == on).all() and by_vertex["kept"][on].all()
    ht, hv = by_table["count"][..., 0] > 0, by_vertex["count"][..., 0] > 0
    agree = float((ht == hv)[on].mean())
    both = on & by_table["window"] & by_vertex["window"]
    dq = np.hypot(by_table["motion"][..., 0] - by_vertex["motion"][..., 0], by_table["motion"][..., 1] - by_vertex["motion"][..., 1])[both]
    print(f"rigid move as a vertex edit: {int(on.sum())} blob pixels, history masks agree on {agree:.4f}, max |dq| {dq.max():.2e} px")
    assert dq.max() <= 1e-3
    # edge pixels: a blob pixel with a neighbour (in either frame's footprint) that is not the blob may flip with the last bit of P'
    edge = np.zeros_like(on)
    prev_on = (prev[2].view(np.int32)[..., 0] == 0) & (prev[1][..., 3] == 3)
    for m in (on, prev_on):
        pad = np.pad(m, 2, constant_values=False)
        for dy in range(5):
            for dx in range(5):
                edge |= ~pad[dy: dy + m.shape[0], dx: dx + m.shape[1]]
    inner = on & ~edge
    assert inner.sum() > 0.3 * on.sum()
    assert (ht == hv)[inner].all()
    assert agree > 0.9
    off = ~on
    for key in ("color", "count", "motion"):                                    # everything else is urt_reproject_objects' to the bit
        assert u32(by_vertex[key])[off].tobytes() == u32(by_table[key])[off].tobytes(), key


# ---- 3. unchanged vertices -------------------------------------------------------------------------------------------------------------------
def test_unchanged_vertices_keep_every_mesh_pixel(mixed):
    sc, aov = mixed
    color, count = history(aov[0].shape[:2])
    Mx = scenes.world_to_clip(sc.camera_to_world, sc.camera_inverse_projection)
    flags = np.ones(len(sc.mesh_objects), np.int32)
    got = reproject_deformed_ref(color, count, *aov, *aov, Mx, sc.camera_to_world, sc.camera_inverse_projection,
                                 deform=(sc.vertices, sc.indices, matrices_of(sc.mesh_objects), flags, -1.0))
    mesh = aov[1][..., 3] == 3
    assert mesh.mean() > 0.03 and (got["deformed"] == mesh).all() and got["kept"][mesh].all()
    P = aov[0][..., :3].astype(np.float64)
    err = np.abs(got["P"].astype(np.float64) - P)[mesh]
    assert (err <= 1e-4 * (1 + np.abs(P[mesh]))).all(), err.max()
    assert (got["count"][..., 0][mesh] > 0).all()
    assert np.abs(got["motion"][..., :2][mesh]).max() < 1e-2                    # nothing moved: the motion vectors say so


# ---- 4. the dead cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["slot -1", "slot past the end", "index outside the vertices", "NaN u", "no area", "object outside the tables"])
def test_dead_cases_give_zeros_and_no_exception(mixed, case):
    sc, aov = mixed
    color, count = history(aov[0].shape[:2])
    Mx = scenes.world_to_clip(sc.camera_to_world, sc.camera_inverse_projection)
    cur = [a.copy() for a in aov]
    ids = cur[2].view(np.int32)
    pv, ix = np.array(sc.vertices, F), np.array(sc.indices, np.int32)
    mats, flags = matrices_of(sc.mesh_objects), flags_for(sc, 0)
    on = (ids[..., 0] == 0) & (cur[1][..., 3] == 3)
    assert on.any()
    if case == "slot -1":
        ids[on, 1] = -1
    elif case == "slot past the end":
        ids[on, 1] = len(ix) - 2
    elif case == "index outside the vertices":
        mo = sc.mesh_objects[0]
        ix[int(mo["indices_offset"]): int(mo["indices_offset"]) + int(mo["indices_count"]): 3] = len(pv)
    elif case == "NaN u":
        cur[2][on, 2] = np.nan
    elif case == "no area":
        lo, hi = blob_span(sc)
        pv[lo: hi + 1] = pv[lo]
    else:
        mats, flags = matrices_of(sc.mesh_objects)[1:2], np.ones(1, np.int32)    # a table of one entry; and the blob's pixels name object 7
        ids[on, 0] = 7
    got = reproject_deformed_ref(color, count, *aov, *cur, Mx, sc.camera_to_world, sc.camera_inverse_projection,
                                 deform=(pv, ix, mats, flags, -1.0))
    for key in ("color", "count", "motion"):
        assert (got[key][on] == 0).all(), key
    assert not got["kept"][on].any()
    others = ~on & (cur[1][..., 3] != 3)
    assert (got["count"][..., 0][others] > 0).mean() > 0.9                       # everything else keeps its history


# ---- 5. the quality move ------------------------------------------------------------------------------------------------------------------------
def test_the_quality_move_covers_enough_and_keeps_enough():
    w, h = QUALITY_SIZE
    sc = scenes.mixed_test_scene(w, h, blob=QUALITY_BLOB)
    cam = scenes.camera_matrices(w, h, position=QUALITY_CAMERA)
    lo, hi = blob_span(sc)
    verts = []
    for phase in QUALITY_PHASE:
        v = np.array(sc.vertices, F)
        v[lo: hi + 1] = scenes.uv_blob(*QUALITY_BLOB, phase=phase)[0]
        verts.append(v)
    assert np.array_equal(verts[0], np.asarray(sc.vertices, F))
    prev, cur = cast(sc, verts[0], size=(w, h), cam=cam), cast(sc, verts[1], size=(w, h), cam=cam)
    color, count = history((h, w))
    got = reproject_deformed_ref(color, count, *prev, *cur, scenes.world_to_clip(*cam), *cam,
                                 deform=(verts[0], sc.indices, matrices_of(sc.mesh_objects), flags_for(sc, QUALITY_MESH)))
    on = (cur[2].view(np.int32)[..., 0] == QUALITY_MESH) & (cur[1][..., 3] == 3)
    cover, kept = float(on.mean()), float((got["count"][..., 0][on] > 0).mean())
    step = np.hypot(got["motion"][..., 0], got["motion"][..., 1])[on & got["window"]]
    print(f"quality move: coverage {cover:.3f}, share with history {kept:.3f}, motion mean {step.mean():.2f} px, max {step.max():.2f} px")
    assert cover >= 1.5 * QUALITY_MIN_COVERAGE, cover                             # room to spare
    assert kept >= QUALITY_MIN_KEPT + 0.2, kept
    assert step.max() > 0.5                                                     # the step does move the surface on screen
