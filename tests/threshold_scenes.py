"""Scenes whose table sizes sit exactly on one side of a layout switch of the default trace kernel (csrc/frame_batch.cpp
configure_sched_at, csrc/scene_prep.cpp prepare_scene): n spheres, n multi-leaf MeshObjects, single-leaf MeshObjects whose triangles sum to
a given total.  Every scene is seen from straight above by a camera that the objects fill, so that a wrong entry of a root table, of a
heap or of the small-triangle copy changes pixels: tests/test_threshold_scenes.py holds each scene to that on the oracle alone, and
tests/test_gpu_table_thresholds.py renders them.  CASES names every scene the GPU tests use, with the sizes the case is about."""
import math

import numpy as np

from unityraytracer_amd import scenes

FOV = 60.0
CELL = 1.3          # grid pitch of the MeshObjects; an object is 1.24 across at the most
TOP = 1.3           # no MeshObject is higher than this; a sphere can reach 2


def _look_down(width, height, x0, x1, z0, z1, top=TOP):
    """Camera above the middle of [x0, x1] x [z0, z1], looking straight down, as low as shows the whole rectangle at height `top`."""
    t = math.tan(math.radians(FOV) * 0.5)
    half = max((z1 - z0) * 0.5, (x1 - x0) * 0.5 * height / width)
    return scenes.camera_matrices(width, height, position=((x0 + x1) * 0.5, top + half / t, (z0 + z1) * 0.5), fov_deg=FOV, pitch_deg=90.0)


def _material(rng, k):
    col = (0.2 + 0.8 * rng.value(), 0.2 + 0.8 * rng.value(), 0.2 + 0.8 * rng.value())
    metal = k % 3 == 0
    return scenes._params((0, 0, 0) if metal else col, col if metal else (0.04, 0.04, 0.04), (2.0, 1.5, 1.0) if k % 7 == 3 else (0, 0, 0), rng.value())


def _fan(k):
    """A flat k-triangle mesh in the plane y = 0 that faces up: k = 2 a quad, else a fan round the centre of a regular k-gon."""
    if k == 2:
        v, t = scenes.quad((-0.5, 0, -0.5), (0.5, 0, -0.5), (0.5, 0, 0.5), (-0.5, 0, 0.5))
    else:
        a = 2.0 * np.pi * np.arange(k) / k
        v = np.concatenate([np.zeros((1, 3)), np.stack([0.55 * np.cos(a), np.zeros(k), 0.55 * np.sin(a)], axis=1)]).astype(np.float32)
        t = np.array([[0, 1 + i, 1 + (i + 1) % k] for i in range(k)], np.int32)
    p = v.astype(np.float64)
    if not scenes.front_facing(p[t[0, 0]], p[t[0, 1]], p[t[0, 2]], np.array([0.0, -1.0, 0.0])):
        t = t[:, [0, 2, 1]]
    return v, t


def _grid(n, cols):
    """Cell centres (x, z) of objects 0 .. n-1, row by row from the far row, columns left to right; and the rectangle they take."""
    rows = -(-n // cols)
    xz = [((i % cols + 0.5) * CELL, (rows - i // cols - 0.5) * CELL) for i in range(n)]
    return xz, (0.0, cols * CELL, 0.0, rows * CELL)


def _scene(name, w, h, b, rect, spheres=None):
    kw = {}
    if b is not None:
        mo, vv, ii, nn, bvh = b.finish()
        kw.update(mesh_objects=mo, vertices=vv, indices=ii, normals=nn, mesh_bvh=bvh)
    if spheres is not None and len(spheres):
        kw.update(spheres=spheres, sphere_bvh=scenes.build_object_bvh(*scenes.sphere_bounds(spheres)))
    sc = scenes.Scene(name, w, h, 4, 1, sky=scenes.make_sky(64, 32), **kw)
    sc.camera_to_world, sc.camera_inverse_projection = _look_down(w, h, *rect, top=2.0 if "spheres" in kw else TOP)
    return sc


def _spheres(n, half, stretch, seed, shift_x=0.0):
    """scenes.make_spheres in a square of half-side `half`, stretched along x to the picture's shape and moved by shift_x."""
    sp = scenes.make_spheres(n, half, seed)
    sp["position"][:, 0] = sp["position"][:, 0] * np.float32(stretch) + np.float32(shift_x)
    return sp


def spheres_scene(n, w=97, h=61, seed=0x5F0):
    half = 0.8 * math.sqrt(n)                       # discs of mean area 1.37 on about 4 n: a third of the ground is covered
    st = w / h
    return _scene(f"spheres{n}", w, h, None, (-half * st, half * st, -half, half), _spheres(n, half, st, seed + n))


def meshes_scene(n, w=97, h=61, n_spheres=0, seed=0x3E5):
    """n level-0 icospheres (20 triangles: a triangle BVH with interior nodes at every leaf size up to 8) on a grid seen from above.  With
    n_spheres, the MeshObjects stand in columns left of the spheres' rectangle."""
    rng = scenes.SplitMix64(seed + 131 * n + n_spheres)
    v, t = scenes.icosphere(0)
    b = scenes.MeshSceneBuilder()
    if n_spheres:
        half = 0.8 * math.sqrt(n_spheres)
        rows = int(2 * half / CELL)
        cols = -(-n // rows)
        rows = -(-n // cols)
    else:
        cols = max(1, min(n, int(round(math.sqrt(n * w / h)))))
    xz, (x0, x1, z0, z1) = _grid(n, cols)
    for k, (x, z) in enumerate(xz):
        b.add(v, t, scenes.trs(translate=(x, 0.65, z), scale=0.62, yaw_deg=360.0 * rng.value()), _material(rng, k))
    sp = None
    if n_spheres:
        width = 2 * half * w / h - (x1 - x0) - 1.0             # what the MeshObjects leave of a picture 2 * half high
        zc = (z0 + z1) * 0.5
        sp = _spheres(n_spheres, half, width / (2 * half), seed + n_spheres, shift_x=x1 + 1.0 + width * 0.5)
        sp["position"][:, 2] += np.float32(zc)
        x1, z0, z1 = x1 + 1.0 + width, zc - half, zc + half
    return _scene(f"meshes{n}+{n_spheres}", w, h, b, (x0, x1, z0, z1), sp)


def small_tris_scene(n_quads, w=97, h=61, extra_big=0, leaf_max=2, seed=0x51A):
    """n_quads flat MeshObjects of leaf_max triangles each (2: quads; 8: fans of 8), every one a single leaf under "blas_leaf_max" =
    leaf_max: leaf_max * n_quads single-leaf triangles in all.  extra_big icospheres (multi-leaf at every leaf size) go into the middle of
    the object list, so that MeshObjects before and after them are single-leaf."""
    rng = scenes.SplitMix64(seed + 17 * n_quads + extra_big + 1000 * leaf_max)
    fv, ft = _fan(leaf_max)
    iv, it = scenes.icosphere(0)
    n = n_quads + extra_big
    xz, rect = _grid(n, max(1, min(n, int(round(math.sqrt(n * w / h))))))
    b = scenes.MeshSceneBuilder()
    for k, (x, z) in enumerate(xz):
        if n_quads // 2 <= k < n_quads // 2 + extra_big:
            b.add(iv, it, scenes.trs(translate=(x, 0.65, z), scale=0.62, yaw_deg=360.0 * rng.value()), _material(rng, k))
        else:
            b.add(fv, ft, scenes.trs(translate=(x, 0.2 + 0.8 * rng.value(), z), scale=1.1, yaw_deg=360.0 * rng.value()), _material(rng, k))
    return _scene(f"small{n_quads}x{leaf_max}+{extra_big}", w, h, b, rect)


def heap_nodes(n):
    """Nodes of the reference builder's heap over n objects: a complete tree of ceil(log2 n) + 1 levels (RM:683,705)."""
    return 0 if n <= 0 else 1 if n == 1 else (2 << int(math.ceil(math.log2(n)))) - 1


# name -> (scene, MeshObjects, spheres, mesh heap nodes, sphere heap nodes, single-leaf triangles, "blas_leaf_max").  The node counts are
# written out, not computed: they are what each case is about.
CASES = {
    "m1": (lambda: meshes_scene(1, 61, 59), 1, 0, 1, 0, 0, 2),
    "m2": (lambda: meshes_scene(2), 2, 0, 3, 0, 0, 2),
    "m3": (lambda: meshes_scene(3, 97, 37), 3, 0, 7, 0, 0, 2),
    "m4": (lambda: meshes_scene(4), 4, 0, 7, 0, 0, 2),
    "m5": (lambda: meshes_scene(5), 5, 0, 15, 0, 0, 2),
    "m12": (lambda: meshes_scene(12), 12, 0, 31, 0, 0, 2),
    "m13": (lambda: meshes_scene(13), 13, 0, 31, 0, 0, 2),
    "m16": (lambda: meshes_scene(16), 16, 0, 31, 0, 0, 2),
    "m17": (lambda: meshes_scene(17), 17, 0, 63, 0, 0, 2),
    "m16+s129": (lambda: meshes_scene(16, n_spheres=129), 16, 129, 31, 511, 0, 2),
    "m128": (lambda: meshes_scene(128, 128, 80), 128, 0, 255, 0, 0, 2),
    "m129": (lambda: meshes_scene(129, 128, 80), 129, 0, 511, 0, 0, 2),
    "s128": (lambda: spheres_scene(128), 0, 128, 0, 255, 0, 2),
    "s129": (lambda: spheres_scene(129), 0, 129, 0, 511, 0, 2),
    "m3+s257": (lambda: meshes_scene(3, 128, 80, n_spheres=257), 3, 257, 7, 1023, 0, 2),
    "fans8+big": (lambda: small_tris_scene(8, extra_big=1, leaf_max=8), 9, 0, 31, 0, 64, 8),      # (the masked FRONT needs a triangle BVH)
    "fans9+big": (lambda: small_tris_scene(9, extra_big=1, leaf_max=8), 10, 0, 31, 0, 72, 8),
    "quads32": (lambda: small_tris_scene(32), 32, 0, 63, 0, 64, 2),
    "quads33": (lambda: small_tris_scene(33), 33, 0, 127, 0, 66, 2),
    "quads32+big": (lambda: small_tris_scene(32, extra_big=1), 33, 0, 127, 0, 64, 2),
}


def first_hits(sc, orc):
    """(kind, object) per pixel of the pixel-centre camera rays, from the oracle's literal Trace (RS:364-383): kind 0 sky, 1 ground,
    2 sphere, 3 triangle.  The oracle reports where a ray hit, not what: the object is the sphere whose surface the point lies on, or the
    MeshObject whose grid cell it is in (the cells do not overlap)."""
    t = math.tan(math.radians(FOV) * 0.5)
    c2w = np.asarray(sc.camera_to_world, np.float64).reshape(4, 4).T
    X, Y = np.meshgrid(np.arange(sc.width) + 0.5, np.arange(sc.height) + 0.5)
    u, v = X / sc.width * 2 - 1, Y / sc.height * 2 - 1
    d = np.stack([u * t * sc.width / sc.height, v * t, -np.ones_like(u)], axis=-1) @ c2w[:3, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = c2w[:3, 3]
    kind = np.zeros((sc.height, sc.width), np.int32)
    obj = np.full((sc.height, sc.width), -1, np.int32)
    if len(sc.mesh_objects):
        lo, hi = scenes.mesh_bounds(sc.mesh_objects, sc.vertices, sc.indices)
        cen = ((lo.astype(np.float64) + hi) * 0.5)[:, [0, 2]]
    for y in range(sc.height):
        for x in range(sc.width):
            r = orc.trace(o, d[y, x], mode=0)
            kind[y, x] = r["kind"]
            p = r["position"].astype(np.float64)
            if r["kind"] == 2:
                obj[y, x] = int(np.argmin(np.abs(np.linalg.norm(sc.spheres["position"] - p, axis=1) - sc.spheres["radius"])))
            elif r["kind"] == 3:
                obj[y, x] = int(np.argmin(((cen - p[[0, 2]]) ** 2).sum(axis=1)))
    return kind, obj
