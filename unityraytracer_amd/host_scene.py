"""Host-side scene preparation through the C ABI (csrc/host_scene.cpp): the C++ counterparts of what
RayTraceMaster.cs does before it uploads buffers.  No GPU needed."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import UrtError
from .scenes import BVHNODE_DT, MESHOBJECT_DT, SPHERE_DT


def _check(lib, rc):
    if rc != 0:
        raise UrtError(rc, lib.urt_host_last_error().decode())


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a.size else None


def compute_normals(vertices, indices) -> np.ndarray:
    """RayTraceMaster.ComputeNormals (RM:340-368) in O(V + I)."""
    lib = _lib.load()
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    ix = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
    out = np.zeros_like(v)
    _check(lib, lib.urt_host_compute_normals(_p(v), len(v), _p(ix), ix.size, _p(out)))
    return out


def normals_plan(vertices, indices, first: int = 0, count: int | None = None) -> dict:
    """The canonical normals plan of include/urt.h for the served vertices first .. first + count - 1 (urt_debug_build_normals_plan; no
    GPU): ranges (count, 2), entries, tris (n_triangles, 3), max_valence."""
    lib = _lib.load()
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    ix = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
    count = len(v) - int(first) if count is None else int(count)
    sizes = np.zeros(3, dtype=np.int32)
    _check(lib, lib.urt_debug_build_normals_plan(_p(v), len(v), _p(ix), ix.size, int(first), count, None, None, 0, None, 0, _p(sizes)))
    ranges = np.zeros((max(count, 0), 2), dtype=np.int32)
    entries, tris = np.zeros(int(sizes[0]), dtype=np.int32), np.zeros((int(sizes[1]), 3), dtype=np.int32)
    _check(lib, lib.urt_debug_build_normals_plan(_p(v), len(v), _p(ix), ix.size, int(first), count, _p(ranges), _p(entries), entries.size,
                                                 _p(tris), len(tris), _p(sizes)))
    return {"ranges": ranges, "entries": entries, "tris": tris, "max_valence": int(sizes[2])}


def morph_deltas(deltas) -> np.ndarray:
    """`deltas` as a contiguous array of urt_MorphDelta (_lib.MORPH_DELTA_DT): such an array as it is, or a sequence of
    (vertex, target, dp[3], dn[3])."""
    dt = np.dtype(_lib.MORPH_DELTA_DT)
    if isinstance(deltas, np.ndarray) and deltas.dtype == dt:
        return np.ascontiguousarray(deltas).reshape(-1)
    out = np.zeros(len(deltas), dtype=dt)
    for k, (vertex, target, dp, dn) in enumerate(deltas):
        out[k] = (vertex, target, dp, dn)
    return out


def morph_plan(deltas, n_targets: int, first: int, count: int) -> dict:
    """The canonical morph plan of include/urt.h for the served vertices first .. first + count - 1 (urt_debug_build_morph_plan; no
    GPU): ranges (count, 2), order (n_deltas), n_entries, max_valence, n_touched."""
    lib = _lib.load()
    d = morph_deltas(deltas)
    ranges, order = np.zeros((max(int(count), 0), 2), dtype=np.int32), np.zeros(len(d), dtype=np.int32)
    sizes = np.zeros(3, dtype=np.int32)
    _check(lib, lib.urt_debug_build_morph_plan(_p(d), len(d), int(n_targets), int(first), int(count), _p(ranges), _p(order), _p(sizes)))
    return {"ranges": ranges, "order": order, "n_entries": int(sizes[0]), "max_valence": int(sizes[1]), "n_touched": int(sizes[2])}


def mesh_leaf_bounds(mesh_objects, vertices, indices, literal: bool = False) -> np.ndarray:
    """SetupBVHLeaves(List<MeshObject>) (RM:405-433); literal=True keeps the reference's quirks."""
    lib = _lib.load()
    mo = np.ascontiguousarray(mesh_objects)
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    ix = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
    out = np.zeros(len(mo), dtype=BVHNODE_DT)
    _check(lib, lib.urt_host_mesh_leaf_bounds(_p(mo), len(mo), _p(v), len(v), _p(ix), ix.size, 1 if literal else 0, _p(out)))
    return out


def sphere_leaf_bounds(spheres, literal: bool = False) -> np.ndarray:
    """SetupBVHLeaves(List<Sphere>) (RM:436-455); literal=True keeps the inverted boxes."""
    lib = _lib.load()
    sp = np.ascontiguousarray(spheres)
    out = np.zeros(len(sp), dtype=BVHNODE_DT)
    _check(lib, lib.urt_host_sphere_leaf_bounds(_p(sp), len(sp), 1 if literal else 0, _p(out)))
    return out


def build_object_bvh(leaves: np.ndarray, pairing: bool = False) -> np.ndarray:
    """Implicit-heap object BVH in the format CreateBVH emits (RM:681-722) from per-object leaf boxes.  pairing=True runs the
    reference's own builder (SetupBVHRankList / PairBVHBounds / JoinBVH, RM:459-678, restated literally) instead of the median split."""
    lib = _lib.load()
    lv = np.ascontiguousarray(leaves, dtype=BVHNODE_DT)
    n = lib.urt_host_object_bvh_length(len(lv))
    if n < 0:                                                # more than 2^30 leaves: 2^D - 1 has no int (include/urt.h)
        raise UrtError(1, f"CreateBVH: the heap of {len(lv)} objects has no int length")
    out = np.zeros(n, dtype=BVHNODE_DT)
    fn = lib.urt_host_build_object_bvh_pairing if pairing else lib.urt_host_build_object_bvh
    _check(lib, fn(_p(lv), len(lv), _p(out), n))
    return out


def _motion(fn, prev, cur, dt, what: str) -> np.ndarray:
    lib = _lib.load()
    a, b = np.ascontiguousarray(prev, dtype=dt).reshape(-1), np.ascontiguousarray(cur, dtype=dt).reshape(-1)
    if len(a) != len(b):
        raise ValueError(f"{what}: the previous list has {len(a)} objects, the current one {len(b)}")
    out = np.zeros((len(a), 12), dtype=np.float32)
    _check(lib, getattr(lib, fn)(_p(a), _p(b), len(a), _p(out)))
    return out


def mesh_motion(prev, cur) -> np.ndarray:
    """The mesh motion table of Context.reproject (include/urt.h urt_host_mesh_motion) from the MeshObject lists (scenes.MESHOBJECT_DT)
    before and after a move: (n, 12) float32, entry i = current world -> previous world of MeshObject i, the exact identity where the
    matrix did not change."""
    return _motion("urt_host_mesh_motion", prev, cur, MESHOBJECT_DT, "mesh_motion")


def sphere_motion(prev, cur) -> np.ndarray:
    """The same for the sphere lists (scenes.SPHERE_DT): urt_host_sphere_motion."""
    return _motion("urt_host_sphere_motion", prev, cur, SPHERE_DT, "sphere_motion")
