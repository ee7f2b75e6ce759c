"""The GPU refit of moved MeshObjects (csrc/refit.hip), checked on the host builder's trees through its numpy restatement
(tests/refit_ref.py; tests/test_gpu_refit_edges.py checks the library's refitted nodes against it bit for bit), over the poses a Unity
host sends: many MeshObjects at once, mirrors, scale 0 and one flattened axis, far translations and back, scales of 1e3 and 1e-3, an
arbitrary rotation with non-uniform scale, and a run of refits that ends where it began.  After every refit, in float64:
- every vertex r0, r0 + e1, r0 + e2 lies inside every ancestor child box, at least half its MeshObject's pad inside on every face;
- the refitted boxes are their vertices' boxes with their own MeshObject's pad, not looser;
- the centre / half-extent copy the trace kernels read contains every box.
Variants of the restatement with the known ways of getting this wrong (no pad, another MeshObject's pad or the scene's, the deepest level
left out, boxes from w1 / w2 with one ulp of pad) must fail these checks: the negative controls below keep them honest."""
import copy

import numpy as np
import pytest

import refit_ref as R
from unityraytracer_amd import debug_build_blas, scenes

F = np.float32

SCENES = {
    "mixed": lambda: scenes.mixed_test_scene(32, 20, blob=(40, 31)),
    "deep_chain": lambda: scenes.deep_chain_scene(32, 20),
    "many_meshes": lambda: scenes.many_meshes_scene(32, 20, n=128),
    "c5_small": lambda: scenes.config5(32, 20, level=2),
}


def mat4(m16):
    """Unity memory order (column-major) 16 floats -> the 4x4 float64 matrix."""
    return np.asarray(m16, np.float64).reshape(4, 4).T


def m16(m):
    return np.ascontiguousarray(np.asarray(m, np.float64).T.astype(F).reshape(16))


def local(m, s):
    """m followed by a local scale s (applied to the mesh before m): m @ diag(s, 1)."""
    return m16(mat4(m) @ np.diag(list(np.broadcast_to(np.asarray(s, np.float64), 3)) + [1.0]))


def world(m, t=(0, 0, 0), yaw_deg=0.0):
    """A world-space rotation about y (about the MeshObject's own position) then translation t, after m."""
    a = mat4(m)
    c, s = np.cos(np.radians(yaw_deg)), np.sin(np.radians(yaw_deg))
    r = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    out = a.copy()
    out[:3, :3] = r @ a[:3, :3]
    out[:3, 3] = a[:3, 3] + np.asarray(t, np.float64)
    return m16(out)


def pose_steps(sc, seed=0):
    """The pose sequence of the refit tests: a list of (name, {MeshObject: 16-float matrix}) applied one after the other.  `sel` are the
    MeshObjects the single-pose steps move (the first, one in the middle and the last)."""
    rng = np.random.default_rng(seed)
    base = np.asarray(sc.mesh_objects["localToWorldMatrix"], F).reshape(-1, 16).copy()
    n = len(base)
    sel = sorted({0, n // 2, n - 1})
    steps = [("all moved", {m: world(base[m], (0.35, 0.2, -0.25), 9.0 + m % 7) for m in range(n)})]
    steps += [("mirror x", {m: local(base[m], (-1, 1, 1)) for m in sel}),
              ("mirror xyz", {m: local(base[m], -1) for m in sel}),
              ("scale 0", {m: local(base[m], 0) for m in sel}),
              ("axis y 0", {m: local(base[m], (1, 0, 1)) for m in sel}),
              ("far 1e5", {m: world(base[m], (1.0e5, 2.5e4, -6.0e4)) for m in sel}),
              ("back", {m: base[m] for m in sel}),
              ("scale 1e3", {m: local(base[m], 1e3) for m in sel}),
              ("scale 1e-3", {m: local(base[m], 1e-3) for m in sel})]
    q = np.array([0.27, -0.41, 0.18, 0.85])
    q /= np.linalg.norm(q)
    steps.append(("quaternion", {m: scenes.trs_quat(tuple(mat4(base[m])[:3, 3]), q, (0.7, 1.9, 0.4)) for m in sel}))
    for k in range(9):
        steps.append((f"walk {k}", {m: world(base[m], rng.uniform(-0.6, 0.6, 3), rng.uniform(-40, 40)) for m in range(n) if rng.random() < 0.6 or m == k % n}))
    steps.append(("home", {m: base[m] for m in range(n)}))
    return steps


def apply(sc, edits):
    """The scene with the edited matrices (heap rebuilt as RebuildTrees does)."""
    out = copy.copy(sc)
    mo = sc.mesh_objects.copy()
    for k, mat in edits.items():
        mo[k]["localToWorldMatrix"] = mat
    out.mesh_objects = mo
    out.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(mo, sc.vertices, sc.indices))
    return out


_trees = {}


def tree(name):
    if name not in _trees:
        sc = SCENES[name]()
        nodes, tri, root, _, _ = debug_build_blas(sc.mesh_objects, sc.vertices, sc.indices)
        _trees[name] = (sc, nodes, tri, root)
    return _trees[name]


def run_sequence(name, variant=None):
    """Refits the host-built tree through the pose sequence with the restatement (or a variant of it).  -> [(step, check results)]."""
    sc, nodes, tri, root = tree(name)
    out, cur = [], sc
    for step, edits in pose_steps(sc):
        nxt = apply(cur, edits)
        moved = R.moved_meshes(cur, nxt)
        new, pad = R.refit(nxt, nodes, tri, root, moved, variant)
        assert np.array_equal(new[:, 12:16].view(np.uint32), nodes[:, 12:16].view(np.uint32)), (name, step)   # child codes and the rest
        _, node_mesh, _ = R.topology(nodes, root)
        still = (node_mesh >= 0) & ~moved[np.maximum(node_mesh, 0)]
        assert np.array_equal(new[still].view(np.uint32), nodes[still].view(np.uint32)), (name, step)        # unmoved: bit for bit
        out.append((step, moved, R.check_boxes(nxt, new, tri, root, R.pad_of(R.mesh_ext(R.records(nxt, tri), len(nxt.mesh_objects))), tight=moved)))
        cur, nodes = nxt, new
    return out


@pytest.mark.parametrize("name", list(SCENES))
def test_refitted_boxes_hold_their_triangles_with_margin(name):
    res = run_sequence(name)
    for step, moved, r in res:
        assert moved.any() or step == "home", (name, step)
        assert R.failures(r) == 0, (name, step, r)
        assert r["min_margin"] >= 0.5, (name, step, r)
    steps = [s for s, _, _ in res]
    assert {"mirror x", "scale 0", "far 1e5", "scale 1e3"} <= set(steps)
    if name == "many_meshes":
        assert res[0][1].sum() >= 100                                      # one step moves >= 100 MeshObjects


def test_restatement_details():
    """The pieces the GPU tests rely on: mul_m4 is the fma chain, lowest component first (close to, but not, the float64 product rounded
    once), the pad is ext 2^-16 + 1e-30 in float32, and non-finite coordinates do not count towards ext."""
    m = np.arange(16, dtype=F) * F(0.37) + F(0.1)
    p = np.array([[1.3, -2.7, 0.55], [1e5, -1e-3, 7.0]], F)
    got = R.mul_m4(m, p)
    M = mat4(m)
    for i in range(len(p)):
        for r in range(3):
            acc = F(m[r] * p[i, 0])
            acc = R.fma32(m[4 + r], p[i, 1], acc)
            acc = R.fma32(m[8 + r], p[i, 2], acc)
            acc = R.fma32(m[12 + r], F(1), acc)
            assert got[i, r].view(np.uint32) == acc.view(np.uint32)
    exact = p.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    assert np.abs(got - exact).max() <= 1e-6 * np.abs(exact).max()
    assert R.pad_of(F(0)) == F(1e-30) and R.pad_of(F(65536)) == F(1) + F(1e-30)
    assert R.pad_of(F(3.0)).view(np.uint32) == F(F(3.0) * F(2.0 ** -16) + F(1e-30)).view(np.uint32)
    rec = {"w": np.array([[[1, np.inf, 2], [np.nan, -5, 0], [0, 0, 0]]], F), "mesh": np.array([1])}
    assert np.array_equal(R.mesh_ext(rec, 3), np.array([0, 5, 0], F))


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_negative_controls_fail_the_checks(variant):
    """Each variant of the restatement breaks the box rule somewhere over the scenes and poses, and the checks see it."""
    names = [n for n in SCENES if variant not in ("other_pad", "scene_pad") or len(tree(n)[0].mesh_objects) > 1]   # (one MeshObject: its own pad)
    bad = {}
    for name in names:
        for step, _, r in run_sequence(name, variant):
            if R.failures(r):
                bad.setdefault(name, []).append(step)
    assert bad, f"variant {variant} passed every check"
    if variant in ("no_pad", "w_boxes_ulp", "scene_pad"):
        assert len(bad) == len(names), (variant, bad)                      # these are wrong on every scene


@pytest.mark.parametrize("variant", ["no_pad", "skip_deepest", "w_boxes_ulp"])
def test_wrong_boxes_leave_vertices_outside(variant):
    """These variants do not just lose margin: vertices end up outside their boxes.  For w_boxes_ulp they are the reconstructed vertices
    r0 + e1, r0 + e2 that the triangle test uses, which can round away from w1, w2 by more than one ulp of the box."""
    contain = sum(r["contain"] for _, _, r in run_sequence("mixed", variant))
    assert contain > 0
