"""Host-side mirror of the UnityEngine objects RayTraceMaster.cs drives, over the C ABI (include/urt.h).

Same names, argument meaning and failure behaviour as the calls at RayTraceMaster.cs:233-259,
772-845 so that code (and tests) written against the reference's host side read the same here:

    ComputeBuffer(count, stride).SetData(list) / .Release() / .count / .stride        RM:233-252
    ComputeShader.SetMatrix/SetVector/SetFloat/SetInt/SetTexture/SetBuffer/Dispatch   RM:772-810
    RenderTexture(w, h) / .Release() / .width / .height                               RM:824-845
    Material("Hidden/AdditionShader").SetFloat("_Sample", n); Graphics.Blit(...)      RM:813-819

Unity's methods return void and log errors; here a failed call raises UrtError (carrying the C
status and message) — a caller wanting Unity's behaviour catches, logs and continues.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _lib
from ._lib import Counters, UrtError


class Context:
    """One per process and GPU (one-process-per-GPU model).  Owns the HIP stream all work is issued on."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        self._h = C.c_void_p()
        rc = self.lib.urt_context_create(int(device), C.byref(self._h))
        if rc != 0:
            raise UrtError(rc, self.lib.urt_last_error(None).decode())
        self.device = device

    def check(self, rc: int):
        if rc != 0:
            raise UrtError(rc, self.lib.urt_last_error(self._h).decode())

    def close(self):
        if self._h:
            self.lib.urt_context_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def synchronize(self):
        self.check(self.lib.urt_synchronize(self._h))

    def flush(self):
        """Submit deferred (batched) frames to the stream without waiting (include/urt.h urt_flush)."""
        self.check(self.lib.urt_flush(self._h))

    def set_stream(self, hip_stream: int | None):
        self.check(self.lib.urt_context_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def set_option(self, name: str, value: int):
        self.check(self.lib.urt_set_option(self._h, name.encode(), int(value)))

    def counters(self) -> dict:
        c = Counters()
        self.check(self.lib.urt_get_counters(self._h, C.byref(c)))
        return c.as_dict()

    def blas_cache_stats(self) -> tuple:
        """(MeshObject BVHs reused, built) by this context's scene preparations so far."""
        a, b = C.c_uint64(), C.c_uint64()
        self.check(self.lib.urt_debug_blas_cache_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def reset_counters(self):
        self.check(self.lib.urt_reset_counters(self._h))

    def refit_stats(self) -> tuple:
        """(MeshObjects refitted on the GPU, scene preparations done in place) since the context was created."""
        a, b = C.c_uint64(), C.c_uint64()
        self.check(self.lib.urt_debug_refit_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def deform_stats(self) -> dict:
        """In-place updates of changed _Vertices / _Normals since the context was created (include/urt.h urt_debug_deform_stats): deformed
        MeshObjects refitted, MeshObjects whose normals were re-gathered, bytes copied to the device, full preparations forced by
        "refit_rebuild_pct", and the largest cost ratio of the last in-place update."""
        a = (C.c_uint64 * 6)()
        self.check(self.lib.urt_debug_deform_stats(self._h, a))
        return {"deformed": int(a[0]), "renormed": int(a[1]), "bytes_copied": int(a[2]), "forced_rebuilds": int(a[3]),
                "cost_ratio": float(np.array([int(a[4])], dtype=np.uint32).view(np.float32)[0])}

    def scene_cost(self, n_meshes: int) -> np.ndarray:
        """(n_meshes, 2) float32: the surface-area cost of every MeshObject's triangle BVH now, and at the last full preparation
        (include/urt.h urt_debug_scene_cost; prepares a stale scene first)."""
        out = np.zeros((int(n_meshes), 2), dtype=np.float32)
        self.check(self.lib.urt_debug_scene_cost(self._h, out.ctypes.data_as(C.c_void_p), int(n_meshes)))
        return out

    def scene_vertex_spans(self, n_meshes: int) -> tuple:
        """(lo[n_meshes], hi[n_meshes]) int32: the smallest and the largest vertex every MeshObject's index range names, as the prepared
        scene holds them (include/urt.h urt_debug_scene_vertex_spans; prepares a stale scene first).  INT32_MAX / -1: none."""
        lo, hi = np.zeros(int(n_meshes), dtype=np.int32), np.zeros(int(n_meshes), dtype=np.int32)
        self.check(self.lib.urt_debug_scene_vertex_spans(self._h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), int(n_meshes)))
        return lo, hi

    def prepare_stats(self) -> dict:
        """Full preparations since the context was created, those of them option "prepare_device" fed from device memory, the indices one
        work item of the vertex-span kernel scans, and the device time of the last span pass in ms (0 unless "time_dispatch" is on) —
        include/urt.h urt_debug_prepare_stats."""
        a = (C.c_uint64 * 4)()
        self.check(self.lib.urt_debug_prepare_stats(self._h, a))
        return {"full": int(a[0]), "device": int(a[1]), "span_chunk": int(a[2]),
                "span_ms": float(np.array([int(a[3])], dtype=np.uint32).view(np.float32)[0])}

    def skin_vertices(self, rest_vertices, rest_normals, bone_indices, bone_weights, bones, first: int, count: int, dst_vertices,
                      dst_normals=None):
        """Linear blend skinning of elements first .. first + count - 1 on the GPU, into the device mirrors of dst_vertices (and
        dst_normals) — include/urt.h urt_skin_vertices.  Every argument but the range is a ComputeBuffer; rest_normals and dst_normals
        may be None (positions only).  Enqueued on the context's stream; nothing is waited for."""
        handle = functools.partial(_buffer_handle, self, "skin_vertices")
        for name, v in (("first", first), ("count", count)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"skin_vertices: {name} must be an int, not {type(v).__name__}")
        sb = _lib.SkinBuffers(handle(rest_vertices, "rest_vertices"), handle(rest_normals, "rest_normals", True),
                              handle(bone_indices, "bone_indices"), handle(bone_weights, "bone_weights"), handle(bones, "bones"))
        self.check(self.lib.urt_skin_vertices(self._h, C.byref(sb), int(first), int(count), handle(dst_vertices, "dst_vertices"),
                                              handle(dst_normals, "dst_normals", True)))

    def buffer_bounds(self, buffer, first: int = 0, count: int | None = None):
        """(min [3], max [3], n): component-wise bounds over the finite elements first .. first + count - 1 of a stride-12 ComputeBuffer,
        reduced on the GPU from its current contents, and their number (include/urt.h urt_buffer_bounds; synchronises).  No finite element:
        (+inf, -inf, 0)."""
        if not isinstance(buffer, ComputeBuffer):
            raise TypeError(f"buffer_bounds: buffer must be a ComputeBuffer, not {type(buffer).__name__}")
        count = buffer.count - int(first) if count is None else count
        out, n = np.zeros(6, dtype=np.float32), C.c_int()
        self.check(self.lib.urt_buffer_bounds(self._h, buffer.handle, int(first), int(count), out.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out[:3].copy(), out[3:].copy(), n.value

    def _buffer_handles(self, who: str, **buffers):
        out = []
        for name, b in buffers.items():
            if not isinstance(b, ComputeBuffer):
                raise TypeError(f"{who}: {name} must be a ComputeBuffer, not {type(b).__name__}")
            if b.ctx is not self:
                raise ValueError(f"{who}: {name} belongs to another context")
            out.append(b.handle)
        return out

    def mesh_leaf_bounds(self, mesh_objects, vertices, indices, dst_leaves):
        """The world-space leaf box of every MeshObject, computed on the GPU from the current device contents of `vertices` into the
        device side of dst_leaves (stride 28, the count of mesh_objects) — include/urt.h urt_mesh_leaf_bounds_device: what
        host_scene.mesh_leaf_bounds computes, by value.  Enqueued on the context's stream; nothing is waited for."""
        h = self._buffer_handles("mesh_leaf_bounds", mesh_objects=mesh_objects, vertices=vertices, indices=indices, dst_leaves=dst_leaves)
        self.check(self.lib.urt_mesh_leaf_bounds_device(self._h, *h))

    def sphere_leaf_bounds(self, spheres, dst_leaves):
        """The leaf box of every sphere into the device side of dst_leaves (include/urt.h urt_sphere_leaf_bounds_device)."""
        h = self._buffer_handles("sphere_leaf_bounds", spheres=spheres, dst_leaves=dst_leaves)
        self.check(self.lib.urt_sphere_leaf_bounds_device(self._h, *h))

    def build_object_bvh(self, leaves, dst_nodes):
        """The implicit heap of host_scene.build_object_bvh over the device contents of `leaves` (at most _lib.OBJECT_BVH_DEVICE_MAX),
        into the device side of dst_nodes, whose count is host_scene.object_bvh_length(leaves.count) — include/urt.h
        urt_build_object_bvh_device.  Enqueued on the context's stream; nothing is waited for."""
        h = self._buffer_handles("build_object_bvh", leaves=leaves, dst_nodes=dst_nodes)
        self.check(self.lib.urt_build_object_bvh_device(self._h, *h))

    def buffer_state(self, buffer) -> dict:
        """Where a ComputeBuffer's contents live (include/urt.h urt_debug_buffer_state): the element range in which the device mirror is
        newer than the host copy (stale_first > stale_last: none), the mirror's bytes (0: no mirror), and the synchronising downloads of
        this buffer so far."""
        a = (C.c_uint64 * 4)()
        self.check(self.lib.urt_debug_buffer_state(self._h, buffer.handle, a))
        return {"stale_first": int(a[0]), "stale_last": int(a[1]), "mirror_bytes": int(a[2]), "downloads": int(a[3])}

    def normals_plan(self, vertices, indices, first: int = 0, count: int | None = None) -> "NormalsPlan":
        """A NormalsPlan for elements first .. first + count - 1 (default: to the end) of the stride-12 ComputeBuffer `vertices`, welded
        against every index slot of the stride-4 ComputeBuffer `indices` as both are NOW (include/urt.h urt_normals_plan_create; a
        synchronising set-up call)."""
        return NormalsPlan(self, vertices, indices, first, count)

    def morph_plan(self, deltas, n_targets: int, first: int, count: int) -> "MorphPlan":
        """A MorphPlan (blend shapes) for the served vertices first .. first + count - 1: `deltas` is an array of urt_MorphDelta
        (_lib.MORPH_DELTA_DT) or a sequence of (vertex, target, dp[3], dn[3]) with absolute vertex numbers (include/urt.h
        urt_morph_plan_create).  The plan names no buffer."""
        return MorphPlan(self, deltas, n_targets, first, count)

    def serve_stats(self) -> dict:
        """kernel_mode 5 with count_stats: the shared traversal service since the last reset_counters()."""
        a = (C.c_ulonglong * 6)()
        self.check(self.lib.urt_debug_serve_stats(self._h, a))
        k = ("visits", "trips", "lane_trips", "claim_rounds", "claimed", "suspended")
        return dict(zip(k, [int(x) for x in a]))

    def scene_info(self) -> dict:
        """Sizes of the current device scene's triangle BVH and the host time its preparation took (prepares it if stale)."""
        nn, nt, md, ms = C.c_int(), C.c_int(), C.c_int(), C.c_float()
        self.check(self.lib.urt_debug_scene_info(self._h, C.byref(nn), C.byref(nt), C.byref(md), C.byref(ms)))
        return {"n_nodes": nn.value, "n_tris": nt.value, "max_depth": md.value, "prepare_ms": ms.value}

    def launch_info(self) -> dict:
        """The last trace launch (deferred frames are submitted first): kernel instantiation by rocprofv3's name, grid, LDS, batching."""
        li = _lib.LaunchInfo()
        self.check(self.lib.urt_debug_launch_info(self._h, C.byref(li)))
        return li.as_dict()

    def read_scene_blas(self, n_meshes: int):
        """(nodes[n,16], tri_index[n_tris], mesh_root[n_meshes]) of the current device scene, read back from the GPU."""
        info = self.scene_info()
        nodes = np.zeros((info["n_nodes"], 16), dtype=np.float32)
        tri = np.zeros(info["n_tris"], dtype=np.int32)
        root = np.zeros(n_meshes, dtype=np.int32)
        self.check(self.lib.urt_debug_read_scene_blas(self._h, nodes.ctypes.data_as(C.c_void_p), tri.ctypes.data_as(C.c_void_p), root.ctypes.data_as(C.c_void_p)))
        return nodes, tri, root, info

    def read_scene_qnodes(self):
        """(frame[2, 4] f32, nodes[n, 8] u32, in_use) of the current device scene: the quantized triangle-BVH nodes of option "qnodes"
        (include/urt.h urt_debug_read_scene_qnodes), read back from the GPU.  frame[0] = grid origin.xyz, quality; frame[1] = cell.xyz, 0.
        n = 0 (and an empty frame) while the option is 0; in_use says whether the traversal reads them."""
        n, use = C.c_int(), C.c_int()
        self.check(self.lib.urt_debug_read_scene_qnodes(self._h, None, C.byref(n), C.byref(use)))
        buf = np.zeros((2 + 2 * n.value, 4), dtype=np.float32)
        if n.value:
            n2 = C.c_int()
            self.check(self.lib.urt_debug_read_scene_qnodes(self._h, buf.ctypes.data_as(C.c_void_p), C.byref(n2), C.byref(use)))
            assert n2.value == n.value
        return buf[:2].copy(), buf[2:].view(np.uint32).reshape(n.value, 8), bool(use.value)

    def read_scene_cones(self):
        """(words[n_nodes, 2] u32, e1[n_tris, 3] f32, e2[n_tris, 3] f32, in_use) of the current device scene: the normal cones of option
        "blas_cones" (include/urt.h urt_debug_read_scene_cones) and the edges of the leaf-order triangle records they were derived from."""
        info = self.scene_info()
        words = np.zeros((info["n_nodes"], 2), dtype=np.uint32)
        edges = np.zeros((info["n_tris"], 6), dtype=np.float32)
        use = C.c_int()
        self.check(self.lib.urt_debug_read_scene_cones(self._h, words.ctypes.data_as(C.c_void_p), edges.ctypes.data_as(C.c_void_p), C.byref(use)))
        return words, edges[:, :3].copy(), edges[:, 3:].copy(), bool(use.value)

    def read_tile_entry(self):
        """(table[tiles_y, tiles_x, k] i32, builds) — the tile entry table of option "tile_entry" as the last launch that used one read it
        (include/urt.h urt_debug_read_tile_entry): per 8x8 tile of the image the node codes its camera rays start from, padded with
        -2^31; an empty (0, 0, 0) array while the context holds no table.  builds: tables built since the context was created."""
        tx, ty, k, builds = C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
        self.check(self.lib.urt_debug_read_tile_entry(self._h, None, 0, C.byref(tx), C.byref(ty), C.byref(k), C.byref(builds)))
        table = np.zeros((ty.value, tx.value, k.value), dtype=np.int32)
        if table.size:
            self.check(self.lib.urt_debug_read_tile_entry(self._h, table.ctypes.data_as(C.c_void_p), table.size, None, None, None, None))
        return table, builds.value

    def ray_query(self, origins, directions, t_max=None, any_hit: bool = False):
        """Batched ray queries against the bound scene (include/urt.h urt_ray_query): what the frame kernels' Trace (RS:364-383)
        returns for each ray, bounded by t_max (exclusive; None = +inf; a scalar or one value per ray).

        numpy float32 arrays (n, 3): returns a RAYHIT_DT structured array (n,), or int32 (n,) occlusion flags with any_hit.
        torch float32 tensors (n, 3) on this context's device: the device entry point on device-resident rays; returns a dict of
        tensor views (distance, position, normal, kind, object, primitive, u, v), or an int32 tensor with any_hit.  The call is
        ordered after torch's current stream and has completed when it returns."""
        if _is_torch(origins) or _is_torch(directions):
            return self._ray_query_torch(origins, directions, t_max, any_hit)
        o = _rays_arg(origins, "origins")
        d = _rays_arg(directions, "directions")
        if o.shape != d.shape:
            raise ValueError(f"ray_query: origins {o.shape} and directions {d.shape} differ in shape")
        n = o.shape[0]
        tm = _t_max_arg(t_max, n)
        rays = np.zeros(n, dtype=RAY_DT)
        rays["origin"], rays["t_max"], rays["direction"] = o, tm, d
        out = np.zeros(n, dtype=np.int32 if any_hit else RAYHIT_DT)
        flags = _lib.URT_QUERY_ANY if any_hit else _lib.URT_QUERY_CLOSEST
        self.check(self.lib.urt_ray_query(self._h, rays.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p), flags))
        return out

    def _ray_query_torch(self, origins, directions, t_max, any_hit):
        import torch
        for name, a in (("origins", origins), ("directions", directions)):
            if not _is_torch(a):
                raise TypeError(f"ray_query: {name} must be a torch tensor when the other one is")
            if a.dtype != torch.float32:
                raise TypeError(f"ray_query: {name} must be float32, not {a.dtype}")
            if a.dim() != 2 or a.shape[1] != 3:
                raise ValueError(f"ray_query: {name} must have shape (n, 3), not {tuple(a.shape)}")
            if a.device.type != "cuda" or a.device.index != self.device:
                raise ValueError(f"ray_query: {name} must be on cuda:{self.device}, not {a.device}")
        if origins.shape != directions.shape:
            raise ValueError(f"ray_query: origins {tuple(origins.shape)} and directions {tuple(directions.shape)} differ in shape")
        n = origins.shape[0]
        if n > 0x7fffffff:
            raise ValueError("ray_query: more than 2^31 - 1 rays")
        if t_max is None:
            tm = torch.full((n, 1), float("inf"), dtype=torch.float32, device=origins.device)
        elif _is_torch(t_max):
            if t_max.dtype != torch.float32 or t_max.shape != (n,) or t_max.device != origins.device:
                raise ValueError("ray_query: t_max must be a float32 tensor of shape (n,) on the rays' device")
            tm = t_max.reshape(n, 1)
        else:
            tm = torch.full((n, 1), float(np.float32(t_max)), dtype=torch.float32, device=origins.device)
        rays = torch.cat([origins, tm, directions, torch.zeros((n, 1), dtype=torch.float32, device=origins.device)], dim=1).contiguous()
        out = torch.empty(n if any_hit else (n, 12), dtype=torch.int32 if any_hit else torch.float32, device=origins.device)
        # the rays are written on torch's current stream, the query runs on the library's: order them (as gather_converged does)
        torch.cuda.current_stream(origins.device).synchronize()
        flags = _lib.URT_QUERY_ANY if any_hit else _lib.URT_QUERY_CLOSEST
        self.check(self.lib.urt_ray_query_device(self._h, C.c_void_p(rays.data_ptr()), n, C.c_void_p(out.data_ptr()), flags))
        torch.cuda.synchronize(origins.device)                   # the device entry point returns at once: wait for the library's stream
        if any_hit:
            return out
        bits = out.view(torch.int32)
        return {"distance": out[:, 0], "position": out[:, 1:4], "normal": out[:, 4:7], "kind": bits[:, 7], "object": bits[:, 8],
                "primitive": bits[:, 9], "u": out[:, 10], "v": out[:, 11]}

    def radiance_query(self, origins, directions, pixels, seeds, samples: int, bounces: int):
        """Path-traced radiance arriving along each ray (include/urt.h urt_radiance_query, URT_RADIANCE_RAYS): `samples` paths of up to
        `bounces` bounces per ray with the bound scene's materials, emission and sky, averaged.  origins, directions (n, 3); pixels (n, 2):
        the two floats that select each query's random stream (the "pixel" of rand(), RS:77-81); seeds: the running seed each query starts
        from, a number or (n,).  numpy float32 arrays: returns (n, 4) float32.  torch float32 tensors on this context's device: the device
        entry point; returns an (n, 4) tensor.  The call is ordered after torch's current stream and has completed when it returns."""
        samples, bounces = _radiance_counts(samples, bounces)
        if any(_is_torch(a) for a in (origins, directions, pixels)):
            return self._radiance_query_torch(origins, directions, pixels, seeds, samples, bounces)
        o = _rays_arg(origins, "origins", "radiance_query")
        d = _rays_arg(directions, "directions", "radiance_query")
        if o.shape != d.shape:
            raise ValueError(f"radiance_query: origins {o.shape} and directions {d.shape} differ in shape")
        n = o.shape[0]
        if not isinstance(pixels, np.ndarray):
            raise TypeError(f"radiance_query: pixels must be a numpy array (or a torch tensor), not {type(pixels).__name__}")
        if pixels.dtype != np.float32:
            raise TypeError(f"radiance_query: pixels must be float32, not {pixels.dtype}")
        if pixels.shape != (n, 2):
            raise ValueError(f"radiance_query: pixels must have shape ({n}, 2), not {pixels.shape}")
        rays = np.zeros(n, dtype=PATHRAY_DT)
        rays["origin"], rays["direction"], rays["seed"] = o, d, _per_ray_arg(seeds, n, "seeds", "radiance_query")
        rays["px"], rays["py"] = pixels[:, 0], pixels[:, 1]
        out = np.zeros((n, 4), dtype=np.float32)
        self.check(self.lib.urt_radiance_query(self._h, rays.ctypes.data_as(C.c_void_p), n, samples, bounces, out.ctypes.data_as(C.c_void_p),
                                               _lib.URT_RADIANCE_RAYS))
        return out

    def _radiance_query_torch(self, origins, directions, pixels, seeds, samples, bounces):
        import torch
        for name, a, cols in (("origins", origins, 3), ("directions", directions, 3), ("pixels", pixels, 2)):
            self._torch_arg(a, name, "radiance_query", torch.float32, cols)
        n = origins.shape[0]
        if directions.shape[0] != n or pixels.shape[0] != n:
            raise ValueError(f"radiance_query: origins {tuple(origins.shape)}, directions {tuple(directions.shape)} and pixels "
                             f"{tuple(pixels.shape)} differ in length")
        if n > 0x7fffffff:
            raise ValueError("radiance_query: more than 2^31 - 1 rays")
        if _is_torch(seeds):
            if seeds.dtype != torch.float32 or seeds.shape != (n,) or seeds.device != origins.device:
                raise ValueError("radiance_query: seeds must be a float32 tensor of shape (n,) on the rays' device")
            sd = seeds.reshape(n, 1)
        else:
            if isinstance(seeds, (bool, np.bool_)) or not isinstance(seeds, (int, float, np.floating, np.integer)):
                raise TypeError(f"radiance_query: seeds must be a number or a float32 tensor, not {type(seeds).__name__}")
            sd = torch.full((n, 1), float(np.float32(seeds)), dtype=torch.float32, device=origins.device)
        zero = torch.zeros((n, 1), dtype=torch.float32, device=origins.device)
        rays = torch.cat([origins, sd, directions, zero, pixels, zero, zero], dim=1).contiguous()
        out = torch.empty((n, 4), dtype=torch.float32, device=origins.device)
        torch.cuda.current_stream(origins.device).synchronize()    # the rays are written on torch's stream, the query runs on the library's
        self.check(self.lib.urt_radiance_query_device(self._h, C.c_void_p(rays.data_ptr()), n, samples, bounces, C.c_void_p(out.data_ptr()),
                                                      _lib.URT_RADIANCE_RAYS))
        torch.cuda.synchronize(origins.device)                     # the device entry point returns at once: wait for the library's stream
        return out

    def radiance_query_pixels(self, xy, samples: int, bounces: int):
        """What a frame dispatched now with _numRays = samples and _numBounces = bounces would write to the given pixels of the texture
        bound as Result (include/urt.h urt_radiance_query, URT_RADIANCE_PIXELS): the camera, _PixelOffset and _Seed bound at call time.
        xy: (n, 2) int32, numpy — returns (n, 4) float32 and refuses pixels outside the texture — or a torch tensor on this context's
        device: the device entry point, which gives (0, 0, 0, 0) to a pixel outside the texture; returns an (n, 4) tensor."""
        samples, bounces = _radiance_counts(samples, bounces)
        if _is_torch(xy):
            import torch
            self._torch_arg(xy, "xy", "radiance_query_pixels", torch.int32, 2)
            n = xy.shape[0]
            if n > 0x7fffffff:
                raise ValueError("radiance_query_pixels: more than 2^31 - 1 pixels")
            px = xy.contiguous()
            out = torch.empty((n, 4), dtype=torch.float32, device=xy.device)
            torch.cuda.current_stream(xy.device).synchronize()
            self.check(self.lib.urt_radiance_query_device(self._h, C.c_void_p(px.data_ptr()), n, samples, bounces, C.c_void_p(out.data_ptr()),
                                                          _lib.URT_RADIANCE_PIXELS))
            torch.cuda.synchronize(xy.device)
            return out
        if not isinstance(xy, np.ndarray):
            raise TypeError(f"radiance_query_pixels: xy must be a numpy array (or a torch tensor), not {type(xy).__name__}")
        if xy.dtype != np.int32:
            raise TypeError(f"radiance_query_pixels: xy must be int32, not {xy.dtype}")
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError(f"radiance_query_pixels: xy must have shape (n, 2), not {xy.shape}")
        if xy.shape[0] > 0x7fffffff:
            raise ValueError("radiance_query_pixels: more than 2^31 - 1 pixels")
        px = np.ascontiguousarray(xy)
        out = np.zeros((len(px), 4), dtype=np.float32)
        self.check(self.lib.urt_radiance_query(self._h, px.ctypes.data_as(C.c_void_p), len(px), samples, bounces, out.ctypes.data_as(C.c_void_p),
                                               _lib.URT_RADIANCE_PIXELS))
        return out

    def _torch_arg(self, a, name: str, who: str, dtype, cols: int):
        if not _is_torch(a):
            raise TypeError(f"{who}: {name} must be a torch tensor when another argument is")
        if a.dtype != dtype:
            raise TypeError(f"{who}: {name} must be {str(dtype).replace('torch.', '')}, not {a.dtype}")
        if a.dim() != 2 or a.shape[1] != cols:
            raise ValueError(f"{who}: {name} must have shape (n, {cols}), not {tuple(a.shape)}")
        if a.device.type != "cuda" or a.device.index != self.device:
            raise ValueError(f"{who}: {name} must be on cuda:{self.device}, not {a.device}")

    def render_aov(self, hit=None, normal=None, albedo=None, id=None, frame_ray: bool = False):
        """Per-pixel first-hit feature buffers of the bound camera into RenderTextures of one size (include/urt.h urt_render_aov):
        hit = position.xyz, distance; normal = normal.xyz, kind; albedo = clamped albedo.xyz, smoothness (a miss: sky radiance, 0);
        id = object, primitive (int32 bits), u, v.  None = not wanted.  frame_ray: the first camera ray of a frame dispatched now instead
        of the pixel centre.  Enqueued on the context's stream after the deferred frames; a later GetPixels sees the result."""
        targets = (("hit", hit), ("normal", normal), ("albedo", albedo), ("id", id))
        for name, t in targets:
            if t is not None and not isinstance(t, RenderTexture):
                raise TypeError(f"render_aov: {name} must be a RenderTexture or None, not {type(t).__name__}")
            if t is not None and t.ctx is not self:
                raise ValueError(f"render_aov: {name} belongs to another context")
            if t is not None and not t.handle:
                raise ValueError(f"render_aov: {name} was released")
        if all(t is None for _, t in targets):
            raise ValueError("render_aov: no target given")
        if not isinstance(frame_ray, (bool, np.bool_)):
            raise TypeError(f"render_aov: frame_ray must be a bool, not {type(frame_ray).__name__}")
        flags = _lib.URT_AOV_FRAME_RAY if frame_ray else _lib.URT_AOV_PIXEL_CENTER
        h = [t.handle if t is not None else 0 for _, t in targets]
        self.check(self.lib.urt_render_aov(self._h, h[0], h[1], h[2], h[3], flags))

    def render_aov_arrays(self, width: int, height: int, frame_ray: bool = False) -> dict:
        """render_aov into four temporary width x height textures, read back as numpy arrays indexed [y, x] (row 0 = bottom):
        position (h, w, 3), distance, normal (h, w, 3), kind (int32), albedo (h, w, 3), smoothness, object and primitive (int32), u, v."""
        width, height = int(width), int(height)
        if width <= 0 or height <= 0:
            raise ValueError(f"render_aov_arrays: size must be positive, not {width} x {height}")
        tex = [RenderTexture(self, width, height) for _ in range(4)]
        try:
            self.render_aov(*tex, frame_ray=frame_ray)
            hit, nrm, alb, ids = (t.GetPixels() for t in tex)
        finally:
            for t in tex:
                t.Release()
        bits = ids.view(np.int32)
        return {"position": hit[..., :3], "distance": hit[..., 3], "normal": nrm[..., :3], "kind": nrm[..., 3].astype(np.int32),
                "albedo": alb[..., :3], "smoothness": alb[..., 3], "object": bits[..., 0].copy(), "primitive": bits[..., 1].copy(),
                "u": ids[..., 2], "v": ids[..., 3]}

    def denoise(self, src, dst, hit, normal, albedo=None, iterations: int = _lib.DENOISE_DEFAULTS["iterations"],
                sigma_color: float = _lib.DENOISE_DEFAULTS["sigma_color"], sigma_normal: float = _lib.DENOISE_DEFAULTS["sigma_normal"],
                sigma_depth: float = _lib.DENOISE_DEFAULTS["sigma_depth"]):
        """Edge-aware a-trous denoise of src's colour into dst, guided by the hit and normal feature buffers of render_aov and optionally
        by albedo (include/urt.h urt_denoise).  RenderTextures of one size; dst may be src.  A sigma <= 0 leaves its term out.  Enqueued on
        the context's stream after the deferred frames; a later GetPixels sees the result."""
        targets = (("src", src), ("dst", dst), ("hit", hit), ("normal", normal), ("albedo", albedo))
        for name, t in targets:
            if t is None and name == "albedo":
                continue
            if not isinstance(t, RenderTexture):
                raise TypeError(f"denoise: {name} must be a RenderTexture{' or None' if name == 'albedo' else ''}, not {type(t).__name__}")
            if t.ctx is not self:
                raise ValueError(f"denoise: {name} belongs to another context")
            if not t.handle:
                raise ValueError(f"denoise: {name} was released")
            if (t.width, t.height) != (src.width, src.height):
                raise ValueError(f"denoise: {name} is {t.width} x {t.height}, src is {src.width} x {src.height}")
        if any(dst is t for t in (hit, normal, albedo)):
            raise ValueError("denoise: dst is one of the guide textures")
        p = denoise_params(iterations, sigma_color, sigma_normal, sigma_depth)
        self.check(self.lib.urt_denoise(self._h, src.handle, dst.handle, hit.handle, normal.handle, albedo.handle if albedo is not None else 0,
                                        C.byref(p)))

    def denoise_arrays(self, color, hit, normal, albedo=None, **params) -> np.ndarray:
        """denoise on numpy images (h, w, 4) float32, row 0 = bottom (the layouts of render_aov: hit.w = distance, normal.w = kind,
        albedo.rgb), through temporary textures; returns the denoised (h, w, 4) image."""
        imgs = [np.ascontiguousarray(a, dtype=np.float32) for a in (color, hit, normal) + ((albedo,) if albedo is not None else ())]
        shape = imgs[0].shape
        if len(shape) != 3 or shape[2] != 4 or shape[0] <= 0 or shape[1] <= 0:
            raise ValueError(f"denoise_arrays: color must be (h, w, 4), not {shape}")
        for a in imgs[1:]:
            if a.shape != shape:
                raise ValueError(f"denoise_arrays: the images differ in shape ({a.shape} vs {shape})")
        h, w = shape[:2]
        tex = []
        try:
            for a in imgs + [None]:
                tex.append(RenderTexture(self, w, h))
                if a is not None:
                    tex[-1].SetPixels(a)
            src, hit_t, nrm_t = tex[:3]
            alb_t = tex[3] if albedo is not None else None
            out = tex[-1]
            self.denoise(src, out, hit_t, nrm_t, alb_t, **params)
            return out.GetPixels()
        finally:
            for t in tex:
                t.Release()

    REPROJECT_INPUTS = ("prev_color", "prev_count", "prev_hit", "prev_normal", "prev_id", "hit", "normal", "id")

    def reproject(self, prev_color, prev_count, prev_hit, prev_normal, prev_id, hit, normal, id, color, count, prev_world_to_clip,
                  motion=None, max_history: float = _lib.REPROJECT_DEFAULTS["max_history"],
                  normal_threshold: float = _lib.REPROJECT_DEFAULTS["normal_threshold"],
                  plane_threshold: float = _lib.REPROJECT_DEFAULTS["plane_threshold"], *, mesh_motion=None, sphere_motion=None,
                  moved_max_history: float = 0.0, deform=None):
        """Temporal reprojection (include/urt.h urt_reproject): the history prev_color / prev_count accumulated under the previous camera,
        whose world-to-clip matrix is prev_world_to_clip (16 floats, column-major: scenes.world_to_clip), carried into the current view
        (the bound _CameraToWorld / _CameraInverseProjection) -> color / count, and the optional motion image.  prev_hit / prev_normal /
        prev_id and hit / normal / id are render_aov's pixel-centre buffers under the previous and the current camera.  RenderTextures
        of one size.  Enqueued after the deferred frames; a later GetPixels sees the result.
        mesh_motion / sphere_motion: ComputeBuffers of stride 48 (urt_ObjectMotion: host_scene.mesh_motion / sphere_motion) for objects
        that have moved between the two sets of feature buffers, moved_max_history an extra clamp of the count on their pixels: with
        any of the three given the call is urt_reproject_objects, else urt_reproject.
        deform: the buffers of meshes that changed shape (include/urt.h urt_ReprojectDeform) as a tuple (prev_vertices, indices,
        prev_mesh_objects, deformed[, normal_threshold]) of ComputeBuffers of stride 12 / 4 / 112 / 4, or an object with attributes of
        these names; the threshold defaults to _lib.REPROJECT_DEFORM_NORMAL_THRESHOLD.  Any deform given makes the call
        urt_reproject_deformed."""
        images = dict(zip(self.REPROJECT_INPUTS, (prev_color, prev_count, prev_hit, prev_normal, prev_id, hit, normal, id)))
        images.update(color=color, count=count, motion=motion)
        for name, t in images.items():
            if t is None and name == "motion":
                continue
            _check_texture(self, "reproject", name, t, prev_color, optional=name == "motion")
        outs = [n for n in ("color", "count", "motion") if images[n] is not None]
        for o in outs:
            for name, t in images.items():
                if name != o and t is images[o]:
                    raise ValueError(f"reproject: the output {o} is also {name}")
        p = reproject_params(prev_world_to_clip, max_history, normal_threshold, plane_threshold)
        for name, b in (("mesh_motion", mesh_motion), ("sphere_motion", sphere_motion)):
            if b is None:
                continue
            if not isinstance(b, ComputeBuffer):
                raise TypeError(f"reproject: {name} must be a ComputeBuffer or None, not {type(b).__name__}")
            if b.ctx is not self:
                raise ValueError(f"reproject: {name} belongs to another context")
            if not b.handle:
                raise ValueError(f"reproject: {name} was released")
            if b.stride != C.sizeof(_lib.ObjectMotion):
                raise ValueError(f"reproject: the stride of {name} is {b.stride}, not {C.sizeof(_lib.ObjectMotion)}")
        mmh = _max_history_arg(moved_max_history, "reproject", "moved_max_history")
        de = None if deform is None else _deform_arg(self, deform)
        im = _lib.ReprojectImages(*(images[n].handle if images[n] is not None else 0 for n, _ in _lib.ReprojectImages._fields_))
        if de is not None:
            mo = _lib.ReprojectMotion(mesh_motion.handle if mesh_motion is not None else 0,
                                      sphere_motion.handle if sphere_motion is not None else 0, mmh, 0)
            self.check(self.lib.urt_reproject_deformed(self._h, C.byref(im), C.byref(p), C.byref(mo), C.byref(de)))
            return
        if mesh_motion is None and sphere_motion is None and mmh == 0.0:
            self.check(self.lib.urt_reproject(self._h, C.byref(im), C.byref(p)))
            return
        mo = _lib.ReprojectMotion(mesh_motion.handle if mesh_motion is not None else 0,
                                  sphere_motion.handle if sphere_motion is not None else 0, mmh, 0)
        self.check(self.lib.urt_reproject_objects(self._h, C.byref(im), C.byref(p), C.byref(mo)))

    def reproject_arrays(self, prev_color, prev_count, prev_hit, prev_normal, prev_id, hit, normal, id, prev_world_to_clip,
                         camera_to_world, camera_inverse_projection, motion: bool = True, mesh_motion=None, sphere_motion=None,
                         moved_max_history: float = 0.0, deform=None, **params) -> dict:
        """reproject on numpy images (h, w, 4) float32, row 0 = bottom, through temporary textures.  camera_to_world /
        camera_inverse_projection (16 floats each) are bound as the context's current camera uniforms first (they stay bound).
        mesh_motion / sphere_motion: the motion tables as (n, 12) float32 arrays (n >= 1) or None.  Returns
        {"color", "count"[, "motion"]} as (h, w, 4) arrays.
        deform: (prev_vertices (n, 3) float32, indices (3 t,) int32, prev_mesh_objects (n_objects records of 112 bytes), deformed
        (n_objects,) int32[, normal_threshold]) as arrays, each with at least one element."""
        tables = {}
        deform_arrays = None
        if deform is not None:
            if not isinstance(deform, (tuple, list)) or len(deform) not in (4, 5):
                raise ValueError("reproject_arrays: deform must be (prev_vertices, indices, prev_mesh_objects, deformed[, normal_threshold])")
            pv = np.ascontiguousarray(deform[0], dtype=np.float32)
            ix = np.ascontiguousarray(deform[1], dtype=np.int32).reshape(-1)
            mo = np.ascontiguousarray(deform[2])
            fl = np.ascontiguousarray(deform[3], dtype=np.int32).reshape(-1)
            if pv.ndim != 2 or pv.shape[1] != 3 or len(pv) < 1:
                raise ValueError(f"reproject_arrays: deform prev_vertices must have shape (n, 3) with n >= 1, not {pv.shape}")
            if mo.nbytes == 0 or mo.nbytes % 112:
                raise ValueError(f"reproject_arrays: deform prev_mesh_objects must hold records of 112 bytes, not {mo.nbytes} bytes")
            if ix.size < 1 or fl.size < 1:
                raise ValueError("reproject_arrays: deform indices and deformed need at least one element")
            deform_arrays = ((pv, 12), (ix, 4), (mo, 112), (fl, 4))
        for name, a in (("mesh_motion", mesh_motion), ("sphere_motion", sphere_motion)):
            if a is None:
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 12 or a.shape[0] < 1:
                raise ValueError(f"reproject_arrays: {name} must have shape (n, 12) with n >= 1, not {a.shape}")
            tables[name] = a
        _max_history_arg(moved_max_history, "reproject", "moved_max_history")
        imgs = [np.ascontiguousarray(a, dtype=np.float32) for a in (prev_color, prev_count, prev_hit, prev_normal, prev_id, hit, normal, id)]
        shape = imgs[0].shape
        if len(shape) != 3 or shape[2] != 4 or shape[0] <= 0 or shape[1] <= 0:
            raise ValueError(f"reproject_arrays: prev_color must be (h, w, 4), not {shape}")
        for a in imgs[1:]:
            if a.shape != shape:
                raise ValueError(f"reproject_arrays: the images differ in shape ({a.shape} vs {shape})")
        reproject_params(prev_world_to_clip, **params)
        c2w, invp = _matrix16(camera_to_world, "camera_to_world"), _matrix16(camera_inverse_projection, "camera_inverse_projection")
        h, w = shape[:2]
        tex, bufs, dbufs = [], {}, []
        try:
            for name, a in tables.items():
                bufs[name] = ComputeBuffer(self, len(a), 48)
                bufs[name].SetData(a)
            for a, stride in deform_arrays or ():
                dbufs.append(ComputeBuffer(self, a.nbytes // stride, stride))
                dbufs[-1].SetData(a)
            for a in imgs + [None] * (3 if motion else 2):
                tex.append(RenderTexture(self, w, h))
                if a is not None:
                    tex[-1].SetPixels(a)
            sh = ComputeShader(self)                               # through the wrapper: it remembers what the context last received, and a
            sh.SetMatrix("_CameraToWorld", c2w)                    # later RayTraceMaster on this context skips a matrix only if it really is bound
            sh.SetMatrix("_CameraInverseProjection", invp)
            outs = tex[8:]
            self.reproject(*tex[:8], outs[0], outs[1], prev_world_to_clip, motion=outs[2] if motion else None,
                           moved_max_history=moved_max_history, deform=None if deform is None else tuple(dbufs) + tuple(deform[4:]),
                           **bufs, **params)
            res = {"color": outs[0].GetPixels(), "count": outs[1].GetPixels()}
            if motion:
                res["motion"] = outs[2].GetPixels()
            return res
        finally:
            for t in tex + list(bufs.values()) + dbufs:
                t.Release()

    def blit_add_history(self, src, dst, count, max_history: float = 0.0):
        """The AdditionShader blend of src into dst with the per-pixel sample count of `count` (include/urt.h urt_blit_add_history);
        count.x becomes the samples used plus one.  Deferred with a batched frame as Graphics.Blit with the AdditionShader is."""
        for name, t in (("src", src), ("dst", dst), ("count", count)):
            _check_texture(self, "blit_add_history", name, t, src)
        if src is dst or count is src or count is dst:
            raise ValueError("blit_add_history: src, dst and count must be three different textures")
        _max_history_arg(max_history, "blit_add_history")
        self.check(self.lib.urt_blit_add_history(self._h, src.handle, dst.handle, count.handle, float(max_history)))

    def upsample(self, low_color, low_hit, low_normal, low_id, hit, normal, id, color, count=None, low_count=None, albedo=None,
                 normal_threshold: float = _lib.UPSAMPLE_DEFAULTS["normal_threshold"],
                 plane_threshold: float = _lib.UPSAMPLE_DEFAULTS["plane_threshold"],
                 count_scale: float = _lib.UPSAMPLE_DEFAULTS["count_scale"], wide_fallback: bool = True, sky_from_albedo: bool = False):
        """Guide-driven upsampling (include/urt.h urt_upsample): low_color, traced on a small pixel grid, reconstructed on the full grid
        -> color, by a bilinear gather that takes a low-resolution tap only where low_hit / low_normal / low_id and hit / normal / id —
        render_aov's pixel-centre buffers of one camera on the two grids — show the same surface.  count (optional) receives the
        per-pixel sample count, low_count's (None: 1 per texel) times count_scale; a pixel no tap serves gets colour and count 0
        (resample_below fills those).  wide_fallback: such a pixel first tries the 4 x 4 low texels around it.  sky_from_albedo: a sky
        pixel with a result takes its rgb from albedo (render_aov's miss value, the sky radiance).  The low_* RenderTextures have one
        size, the others another.  Enqueued after the deferred frames; a later GetPixels sees the result."""
        low = {"low_color": low_color, "low_count": low_count, "low_hit": low_hit, "low_normal": low_normal, "low_id": low_id}
        full = {"hit": hit, "normal": normal, "id": id, "albedo": albedo, "color": color, "count": count}
        optional = ("low_count", "albedo", "count")
        for group, like in ((low, low_color), (full, hit)):
            for name, t in group.items():
                if t is None and name in optional:
                    continue
                _check_texture(self, "upsample", name, t, like if isinstance(like, RenderTexture) else t, optional=name in optional)
        images = {**low, **full}
        for o in ("color", "count"):
            for name, t in images.items():
                if images[o] is not None and name != o and t is images[o]:
                    raise ValueError(f"upsample: the output {o} is also {name}")
        p = upsample_params(normal_threshold, plane_threshold, count_scale, wide_fallback, sky_from_albedo)
        im = _lib.UpsampleImages(*(images[n].handle if images[n] is not None else 0 for n, _ in _lib.UpsampleImages._fields_))
        self.check(self.lib.urt_upsample(self._h, C.byref(im), C.byref(p)))

    def auto_exposure(self, src, state, count=None, **params):
        """Meters src into an exposure state (include/urt.h urt_auto_exposure): a 256-bin luminance histogram, four bins per stop, the
        mean bin of the texels whose rank lies between low_permille and high_permille, and the exposure that brings its luminance to
        `key`, clamped to [min_exposure, max_exposure] and approached at `rate` per call (>= 1: at once).  state: a torch tensor on this
        context's device, contiguous, at least 1040 bytes, 16-byte aligned (torch.zeros(260, dtype=torch.int32) is a fresh one); it
        stays on the device — exposure_state downloads it.  count (optional): a count texture of src's size; texels whose count is not
        > 0 are left out.  params: the fields of urt_ExposureParams (_lib.EXPOSURE_DEFAULTS).  Enqueued after the deferred frames."""
        _check_texture(self, "auto_exposure", "src", src, src)
        if count is not None:
            _check_texture(self, "auto_exposure", "count", count, src, optional=True)
        if src.width * src.height > 0x7fffffff:
            raise ValueError("auto_exposure: src has more than 2^31 - 1 texels")
        p = exposure_params(**params)
        ptr = self._state_arg(state, "auto_exposure")
        _sync_torch_stream(state)                                  # the state is written on torch's stream, the metering runs on the library's
        self.check(self.lib.urt_auto_exposure(self._h, src.handle, count.handle if count is not None else 0, C.byref(p), C.c_void_p(ptr)))

    def tonemap(self, src, dst, state=None, **params):
        """dst = operator(src * exposure) per colour channel, alpha copied (include/urt.h urt_tonemap); dst may be src.  state: None, or
        the exposure state auto_exposure wrote, whose exposure multiplies params' on the device (no download).  params: exposure, white,
        op (an int, _lib.URT_TONEMAP_*, or "linear" / "reinhard" / "aces"), flags of urt_TonemapParams (_lib.TONEMAP_DEFAULTS).
        Enqueued after the deferred frames; a later GetPixels or formatted read sees the result."""
        _check_texture(self, "tonemap", "src", src, src)
        _check_texture(self, "tonemap", "dst", dst, src)
        p = tonemap_params(**params)
        ptr = 0
        if state is not None:
            ptr = self._state_arg(state, "tonemap")
            _sync_torch_stream(state)
        self.check(self.lib.urt_tonemap(self._h, src.handle, dst.handle, C.byref(p), C.c_void_p(ptr)))

    def depth_of_field(self, src, hit, dst, **params):
        """dst = src blurred by a thin lens' circle of confusion, alpha copied (include/urt.h urt_depth_of_field).  hit: the hit target of
        render_aov for the same camera (its .w is the distance, +inf for the sky).  A pixel at `focus_distance` is sharp, a point at
        infinity blurs over `scale` pixels (dof_scale derives it from a physical camera), nothing blurs wider than `max_radius` (at most
        _lib.URT_DOF_MAX_RADIUS).  dst is neither src nor hit.  params: the fields of urt_DofParams (_lib.DOF_DEFAULTS); flags
        _lib.URT_DOF_FLAG_COC writes each pixel's blur radius instead of the image.  Enqueued after the deferred frames, ahead of bloom."""
        _check_texture(self, "depth_of_field", "src", src, src)
        _check_texture(self, "depth_of_field", "hit", hit, src)
        _check_texture(self, "depth_of_field", "dst", dst, src)
        if dst is src or dst is hit or dst.handle in (src.handle, hit.handle):
            raise ValueError("depth_of_field: dst is also an input (there is no in-place form)")
        p = dof_params(**params)
        self.check(self.lib.urt_depth_of_field(self._h, src.handle, hit.handle, dst.handle, C.byref(p)))

    def motion_blur(self, src, motion, hit, dst, **params):
        """dst = src streaked along the screen-space motion of the open shutter, alpha copied (include/urt.h urt_motion_blur).  motion:
        the motion image of reproject (the displacement in pixels to where each pixel's point was, .z > 0 where valid); hit: the hit
        target of render_aov for the same camera.  The streak of a pixel is `shutter` times its motion long, at most `max_radius` (at
        most _lib.URT_MOTION_BLUR_MAX_RADIUS) to either side; tiles near which nothing moves half a pixel are copied.  dst is none of
        the inputs.  params: the fields of urt_MotionBlurParams (_lib.MOTION_BLUR_DEFAULTS); flags _lib.URT_MOTION_BLUR_FLAG_VELOCITY
        writes the velocity each pixel is gathered along instead of the image.  Enqueued after the deferred frames, after
        depth_of_field and ahead of bloom."""
        _check_texture(self, "motion_blur", "src", src, src)
        _check_texture(self, "motion_blur", "motion", motion, src)
        _check_texture(self, "motion_blur", "hit", hit, src)
        _check_texture(self, "motion_blur", "dst", dst, src)
        if any(dst is t or dst.handle == t.handle for t in (src, motion, hit)):
            raise ValueError("motion_blur: dst is also an input (there is no in-place form)")
        p = motion_blur_params(**params)
        self.check(self.lib.urt_motion_blur(self._h, src.handle, motion.handle, hit.handle, dst.handle, C.byref(p)))

    def bloom(self, src, dst, state=None, **params):
        """dst = src + intensity * bloom(src) per colour channel, alpha copied (include/urt.h urt_bloom); dst may be src.  The bloom is
        what lies above `threshold` (soft below it over `soft_knee`, held to `clamp`), taken down a pyramid of at most `levels` halved
        levels and back up, each coarser level reaching the next finer one by `scatter`.  state: None, or the exposure state
        auto_exposure wrote: threshold and clamp then count in exposed units, divided by its exposure on the device (no download).
        params: the fields of urt_BloomParams (_lib.BLOOM_DEFAULTS); flags _lib.URT_BLOOM_FLAG_ONLY leaves src out of dst.  Enqueued
        after the deferred frames, ahead of tonemap."""
        _check_texture(self, "bloom", "src", src, src)
        _check_texture(self, "bloom", "dst", dst, src)
        p = bloom_params(**params)
        ptr = 0
        if state is not None:
            ptr = self._state_arg(state, "bloom")
            _sync_torch_stream(state)
        self.check(self.lib.urt_bloom(self._h, src.handle, dst.handle, C.byref(p), C.c_void_p(ptr)))

    def exposure_state(self, state) -> dict:
        """The exposure state downloaded (waits for the context's stream): exposure, target, counted, skipped and hist (256 uint32)."""
        self._state_arg(state, "exposure_state")
        self.synchronize()
        raw = state.detach().contiguous().view(-1).cpu().numpy().view(np.uint8)[:C.sizeof(_lib.ExposureState)]
        s = _lib.ExposureState.from_buffer_copy(raw.tobytes())
        return {"exposure": float(s.exposure), "target": float(s.target), "counted": int(s.counted), "skipped": int(s.skipped),
                "hist": np.array(s.hist, dtype=np.uint32)}

    def _state_arg(self, state, who: str) -> int:
        """The device address of an exposure state: a contiguous torch tensor of >= 1040 bytes on this context's device, 16-byte aligned."""
        if not _is_torch(state):
            raise TypeError(f"{who}: state must be a torch tensor on cuda:{self.device}, not {type(state).__name__}")
        if state.device.type != "cuda" or state.device.index != self.device:
            raise ValueError(f"{who}: state must be on cuda:{self.device}, not {state.device}")
        if not state.is_contiguous():
            raise ValueError(f"{who}: state must be contiguous")
        nbytes = state.numel() * state.element_size()
        if nbytes < C.sizeof(_lib.ExposureState):
            raise ValueError(f"{who}: state holds {nbytes} bytes, a urt_ExposureState has {C.sizeof(_lib.ExposureState)}")
        ptr = state.data_ptr()
        if ptr & 15:
            raise ValueError(f"{who}: state must be 16-byte aligned")
        return ptr

    def select_pixels(self, count, below: float = 1.0):
        """The pixels of the count texture whose count is not >= below (include/urt.h urt_select_pixels), found on the GPU: an (n, 2)
        int32 torch tensor of (x, y) on this context's device, in ascending texel order y * width + x — the list radiance_query_pixels
        and blend_samples take.  NaN and negative counts are selected.  Counts first, then allocates n entries and fills them."""
        _check_texture(self, "select_pixels", "count", count, count)
        below = _number_arg(below, "below", "select_pixels")
        import torch
        dev = torch.device("cuda", self.device)
        n = C.c_int(-1)
        self.check(self.lib.urt_select_pixels(self._h, count.handle, below, None, 0, C.byref(n)))
        xy = torch.empty((n.value, 2), dtype=torch.int32, device=dev)
        if n.value > 0:
            torch.cuda.current_stream(dev).synchronize()           # the allocator may hand out memory torch's stream still works on
            m = C.c_int(-1)
            self.check(self.lib.urt_select_pixels(self._h, count.handle, below, C.c_void_p(xy.data_ptr()), n.value, C.byref(m)))
            if m.value != n.value:
                raise RuntimeError(f"select_pixels: the count texture changed between the two passes ({n.value} then {m.value} pixels)")
        return xy

    def blend_samples(self, xy, samples, dst, count, weight: float = 1.0, max_history: float = 0.0):
        """Blends samples[i] into pixel xy[i] of dst with the per-pixel sample count of `count` (include/urt.h urt_blend_samples): the
        arithmetic of blit_add_history with `weight` frame-equivalents per sample; count.x becomes the samples used plus weight.  xy:
        (n, 2) int32 and samples: (n, 4) float32 torch tensors on this context's device; the pixels must be distinct; one outside dst is
        skipped.  The call is ordered after torch's current stream and has completed when it returns."""
        import torch
        weight = _weight_arg(weight, "blend_samples")
        max_history = _max_history_arg(max_history, "blend_samples")
        for name, t in (("dst", dst), ("count", count)):
            _check_texture(self, "blend_samples", name, t, dst)
        if dst is count:
            raise ValueError("blend_samples: dst and count must be two different textures")
        lists = (("xy", xy, torch.int32, 2), ("samples", samples, torch.float32, 4))
        for name, a, dtype, cols in lists:                         # type, dtype and shape of both lists, then where they live
            if not _is_torch(a):
                raise TypeError(f"blend_samples: {name} must be a torch tensor, not {type(a).__name__}")
            if a.dtype != dtype:
                raise TypeError(f"blend_samples: {name} must be {str(dtype).replace('torch.', '')}, not {a.dtype}")
            if a.dim() != 2 or a.shape[1] != cols:
                raise ValueError(f"blend_samples: {name} must have shape (n, {cols}), not {tuple(a.shape)}")
        for name, a, dtype, cols in lists:
            self._torch_arg(a, name, "blend_samples", dtype, cols)
        n = xy.shape[0]
        if samples.shape[0] != n:
            raise ValueError(f"blend_samples: xy {tuple(xy.shape)} and samples {tuple(samples.shape)} differ in length")
        if n > 0x7fffffff:
            raise ValueError("blend_samples: more than 2^31 - 1 samples")
        px, sm = xy.contiguous(), samples.contiguous()
        torch.cuda.current_stream(xy.device).synchronize()         # the lists are written on torch's stream, the blend runs on the library's
        self.check(self.lib.urt_blend_samples(self._h, C.c_void_p(px.data_ptr() if n else 0), C.c_void_p(sm.data_ptr() if n else 0), n, weight,
                                              dst.handle, count.handle, max_history))
        torch.cuda.synchronize(xy.device)                          # returns at once: wait before torch may free the lists

    def resample_below(self, dst, count, below: float, samples: int, bounces: int, weight: float = 1.0, max_history: float = 0.0) -> int:
        """select_pixels(count, below), radiance_query_pixels over the list with `samples` and `bounces`, blend_samples into dst and count
        — in one call, lists and samples in scratch of the context (include/urt.h urt_resample_below).  dst and count have the size of
        the texture bound as Result; the camera, _PixelOffset and _Seed are those bound at call time.  Returns the number of pixels
        resampled; the trace and the blend are enqueued, a later GetPixels sees them."""
        samples, bounces = _radiance_counts(samples, bounces)
        for name, t in (("dst", dst), ("count", count)):
            _check_texture(self, "resample_below", name, t, dst)
        if dst is count:
            raise ValueError("resample_below: dst and count must be two different textures")
        below = _number_arg(below, "below", "resample_below")
        weight = _weight_arg(weight, "resample_below")
        max_history = _max_history_arg(max_history, "resample_below")
        n = C.c_int(-1)
        self.check(self.lib.urt_resample_below(self._h, dst.handle, count.handle, below, samples, bounces, weight, max_history, C.byref(n)))
        return n.value


def _check_texture(ctx, what: str, name: str, t, like, optional: bool = False):
    if not isinstance(t, RenderTexture):
        raise TypeError(f"{what}: {name} must be a RenderTexture{' or None' if optional else ''}, not {type(t).__name__}")
    if t.ctx is not ctx:
        raise ValueError(f"{what}: {name} belongs to another context")
    if not t.handle:
        raise ValueError(f"{what}: {name} was released")
    if (t.width, t.height) != (like.width, like.height):
        raise ValueError(f"{what}: {name} is {t.width} x {t.height}, not {like.width} x {like.height}")


def _buffer_handle(ctx, what: str, b, name: str, optional: bool = False) -> int:
    """The handle of a ComputeBuffer of ctx (0 for None where that is allowed)."""
    if b is None and optional:
        return 0
    if not isinstance(b, ComputeBuffer):
        raise TypeError(f"{what}: {name} must be a ComputeBuffer{' or None' if optional else ''}, not {type(b).__name__}")
    if b.ctx is not ctx:
        raise ValueError(f"{what}: {name} belongs to another context")
    return b.handle


DEFORM_FIELDS = (("prev_vertices", 12), ("indices", 4), ("prev_mesh_objects", 112), ("deformed", 4))


def _deform_arg(ctx, deform) -> "_lib.ReprojectDeform":
    """The checked urt_ReprojectDeform of Context.reproject: a tuple (prev_vertices, indices, prev_mesh_objects, deformed[,
    normal_threshold]) or an object with these attributes; ComputeBuffers of this context with strides 12 / 4 / 112 / 4, a threshold
    that is a number and not NaN."""
    if isinstance(deform, (tuple, list)):
        if len(deform) not in (4, 5):
            raise ValueError(f"reproject: deform must hold four buffers and, optionally, the normal threshold, not {len(deform)} items")
        bufs = list(deform[:4])
        nt = deform[4] if len(deform) == 5 else None
    else:
        try:
            bufs = [getattr(deform, name) for name, _ in DEFORM_FIELDS]
        except AttributeError:
            raise TypeError(f"reproject: deform must be a tuple of four ComputeBuffers (and a threshold) or an object with the attributes "
                            f"{', '.join(n for n, _ in DEFORM_FIELDS)}, not {type(deform).__name__}") from None
        nt = getattr(deform, "normal_threshold", None)
    for (name, stride), b in zip(DEFORM_FIELDS, bufs):
        if not isinstance(b, ComputeBuffer):
            raise TypeError(f"reproject: deform {name} must be a ComputeBuffer, not {type(b).__name__}")
        if b.ctx is not ctx:
            raise ValueError(f"reproject: deform {name} belongs to another context")
        if not b.handle:
            raise ValueError(f"reproject: deform {name} was released")
        if b.stride != stride:
            raise ValueError(f"reproject: the stride of deform {name} is {b.stride}, not {stride}")
    if bufs[1].count % 3:
        raise ValueError(f"reproject: the count of deform indices ({bufs[1].count}) is not a multiple of 3")
    if bufs[2].count != bufs[3].count:
        raise ValueError(f"reproject: deform prev_mesh_objects holds {bufs[2].count} elements, deformed {bufs[3].count}")
    nt = _number_arg(_lib.REPROJECT_DEFORM_NORMAL_THRESHOLD if nt is None else nt, "deform normal_threshold", "reproject")
    return _lib.ReprojectDeform(*(b.handle for b in bufs), nt, 0)


def _number_arg(v, name: str, what: str) -> float:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise TypeError(f"{what}: {name} must be a number, not {type(v).__name__}")
    if np.isnan(v):
        raise ValueError(f"{what}: {name} is NaN")
    return float(v)


def _max_history_arg(v, what: str, name: str = "max_history") -> float:
    v = _number_arg(v, name, what)
    if not (v == 0.0 or v >= 1.0):
        raise ValueError(f"{what}: {name} must be 0 (unlimited) or >= 1, not {v}")
    return v


def _weight_arg(v, what: str) -> float:
    """weight of urt_blend_samples: finite and > 0."""
    v = _number_arg(v, "weight", what)
    if not (np.isfinite(v) and v > 0.0):
        raise ValueError(f"{what}: weight must be finite and > 0, not {v}")
    return v


def _matrix16(m, name: str) -> np.ndarray:
    if isinstance(m, (str, bytes)):
        raise TypeError(f"{name} must be 16 numbers")
    a = np.ascontiguousarray(m, dtype=np.float32).reshape(-1)
    if a.size != 16:
        raise ValueError(f"{name} must be 16 numbers (a 4 x 4 matrix in column-major order), not {a.size}")
    return a


def reproject_params(prev_world_to_clip, max_history: float = _lib.REPROJECT_DEFAULTS["max_history"],
                     normal_threshold: float = _lib.REPROJECT_DEFAULTS["normal_threshold"],
                     plane_threshold: float = _lib.REPROJECT_DEFAULTS["plane_threshold"]) -> _lib.ReprojectParams:
    """The checked urt_ReprojectParams of Context.reproject: 16 matrix entries, max_history 0 or >= 1, thresholds that are not NaN."""
    m = _matrix16(prev_world_to_clip, "reproject: prev_world_to_clip")
    mh = _max_history_arg(max_history, "reproject")
    nt = _number_arg(normal_threshold, "normal_threshold", "reproject")
    pt = _number_arg(plane_threshold, "plane_threshold", "reproject")
    return _lib.ReprojectParams((C.c_float * 16)(*m.tolist()), mh, nt, pt, 0)


def upsample_params(normal_threshold: float = _lib.UPSAMPLE_DEFAULTS["normal_threshold"],
                    plane_threshold: float = _lib.UPSAMPLE_DEFAULTS["plane_threshold"],
                    count_scale: float = _lib.UPSAMPLE_DEFAULTS["count_scale"], wide_fallback: bool = True,
                    sky_from_albedo: bool = False) -> _lib.UpsampleParams:
    """The checked urt_UpsampleParams of Context.upsample: thresholds that are not NaN, a count_scale that is finite and > 0, two bools."""
    nt = _number_arg(normal_threshold, "normal_threshold", "upsample")
    pt = _number_arg(plane_threshold, "plane_threshold", "upsample")
    cs = _number_arg(count_scale, "count_scale", "upsample")
    if not (np.isfinite(cs) and cs > 0.0):
        raise ValueError(f"upsample: count_scale must be finite and > 0, not {cs}")
    for name, v in (("wide_fallback", wide_fallback), ("sky_from_albedo", sky_from_albedo)):
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError(f"upsample: {name} must be a bool, not {type(v).__name__}")
    flags = (_lib.URT_UPSAMPLE_WIDE_FALLBACK if wide_fallback else 0) | (_lib.URT_UPSAMPLE_SKY_FROM_ALBEDO if sky_from_albedo else 0)
    return _lib.UpsampleParams(nt, pt, cs, flags)


def _float32_arg(v, name: str, what: str) -> float:
    """A number as the float32 the library sees (a value beyond its range becomes inf)."""
    with np.errstate(over="ignore"):
        return float(np.float32(_number_arg(v, name, what)))


def _int_arg(v, name: str, what: str) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{what}: {name} must be an int, not {type(v).__name__}")
    return int(v)


def exposure_params(**params) -> _lib.ExposureParams:
    """The checked urt_ExposureParams of Context.auto_exposure: key, min_exposure <= max_exposure finite and > 0, rate > 0,
    0 <= low_permille < high_permille <= 1000; what is not given is _lib.EXPOSURE_DEFAULTS'."""
    unknown = set(params) - set(_lib.EXPOSURE_DEFAULTS)
    if unknown:
        raise TypeError(f"auto_exposure: unknown parameters {sorted(unknown)}")
    v = {**_lib.EXPOSURE_DEFAULTS, **params}
    for name in ("key", "min_exposure", "max_exposure"):
        v[name] = _float32_arg(v[name], name, "auto_exposure")
        if not (np.isfinite(v[name]) and v[name] > 0.0):
            raise ValueError(f"auto_exposure: {name} must be finite and > 0, not {v[name]}")
    if v["min_exposure"] > v["max_exposure"]:
        raise ValueError(f"auto_exposure: min_exposure {v['min_exposure']} is above max_exposure {v['max_exposure']}")
    v["rate"] = _float32_arg(v["rate"], "rate", "auto_exposure")
    if not v["rate"] > 0.0:
        raise ValueError(f"auto_exposure: rate must be > 0, not {v['rate']}")
    lo, hi = (_int_arg(v[name], name, "auto_exposure") for name in ("low_permille", "high_permille"))
    if not 0 <= lo < hi <= 1000:
        raise ValueError(f"auto_exposure: the permilles must satisfy 0 <= low < high <= 1000, not {lo} and {hi}")
    return _lib.ExposureParams(v["key"], v["min_exposure"], v["max_exposure"], v["rate"], lo, hi)


TONEMAP_OPERATORS = {"linear": _lib.URT_TONEMAP_LINEAR, "reinhard": _lib.URT_TONEMAP_REINHARD, "aces": _lib.URT_TONEMAP_ACES}


def tonemap_params(**params) -> _lib.TonemapParams:
    """The checked urt_TonemapParams of Context.tonemap: exposure finite and > 0, white in [0.01, 65504], a known op (its number or its
    name in TONEMAP_OPERATORS), flags 0; what is not given is _lib.TONEMAP_DEFAULTS'."""
    unknown = set(params) - set(_lib.TONEMAP_DEFAULTS)
    if unknown:
        raise TypeError(f"tonemap: unknown parameters {sorted(unknown)}")
    v = {**_lib.TONEMAP_DEFAULTS, **params}
    exposure = _float32_arg(v["exposure"], "exposure", "tonemap")
    if not (np.isfinite(exposure) and exposure > 0.0):
        raise ValueError(f"tonemap: exposure must be finite and > 0, not {exposure}")
    white = _float32_arg(v["white"], "white", "tonemap")
    if not (np.float32(0.01) <= white <= 65504.0):
        raise ValueError(f"tonemap: white must lie in [0.01, 65504], not {white}")
    op = v["op"]
    if isinstance(op, str):
        if op not in TONEMAP_OPERATORS:
            raise ValueError(f"tonemap: unknown operator {op!r} (one of {sorted(TONEMAP_OPERATORS)})")
        op = TONEMAP_OPERATORS[op]
    op = _int_arg(op, "op", "tonemap")
    if op not in TONEMAP_OPERATORS.values():
        raise ValueError(f"tonemap: unknown op {op}")
    flags = _int_arg(v["flags"], "flags", "tonemap")
    if flags != 0:
        raise ValueError(f"tonemap: flags must be 0, not {flags}")
    return _lib.TonemapParams(exposure, white, op, flags)


def bloom_params(**params) -> _lib.BloomParams:
    """The checked urt_BloomParams of Context.bloom: threshold in [0, 65504], soft_knee and scatter in [0, 1], clamp in (0, 65504],
    intensity finite and >= 0, levels 1..16, flags 0 or _lib.URT_BLOOM_FLAG_ONLY; what is not given is _lib.BLOOM_DEFAULTS'."""
    unknown = set(params) - set(_lib.BLOOM_DEFAULTS)
    if unknown:
        raise TypeError(f"bloom: unknown parameters {sorted(unknown)}")
    v = {**_lib.BLOOM_DEFAULTS, **params}
    for name in ("threshold", "soft_knee", "clamp", "scatter", "intensity"):
        v[name] = _float32_arg(v[name], name, "bloom")
    if not 0.0 <= v["threshold"] <= 65504.0:
        raise ValueError(f"bloom: threshold must lie in [0, 65504], not {v['threshold']}")
    for name in ("soft_knee", "scatter"):
        if not 0.0 <= v[name] <= 1.0:
            raise ValueError(f"bloom: {name} must lie in [0, 1], not {v[name]}")
    if not 0.0 < v["clamp"] <= 65504.0:
        raise ValueError(f"bloom: clamp must lie in (0, 65504], not {v['clamp']}")
    if not (np.isfinite(v["intensity"]) and v["intensity"] >= 0.0):
        raise ValueError(f"bloom: intensity must be finite and >= 0, not {v['intensity']}")
    levels, flags = (_int_arg(v[name], name, "bloom") for name in ("levels", "flags"))
    if not 1 <= levels <= 16:
        raise ValueError(f"bloom: levels must be 1..16, not {levels}")
    if flags & ~_lib.URT_BLOOM_FLAG_ONLY:
        raise ValueError(f"bloom: unknown flag bits in {flags}")
    return _lib.BloomParams(v["threshold"], v["soft_knee"], v["clamp"], v["scatter"], v["intensity"], levels, flags)


def dof_params(**params) -> _lib.DofParams:
    """The checked urt_DofParams of Context.depth_of_field: focus_distance finite and > 0, scale finite and >= 0, max_radius in
    [0.5, 16], flags 0 or _lib.URT_DOF_FLAG_COC; what is not given is _lib.DOF_DEFAULTS'."""
    unknown = set(params) - set(_lib.DOF_DEFAULTS)
    if unknown:
        raise TypeError(f"depth_of_field: unknown parameters {sorted(unknown)}")
    v = {**_lib.DOF_DEFAULTS, **params}
    for name in ("focus_distance", "scale", "max_radius"):
        v[name] = _float32_arg(v[name], name, "depth_of_field")
    if not (np.isfinite(v["focus_distance"]) and v["focus_distance"] > 0.0):
        raise ValueError(f"depth_of_field: focus_distance must be finite and > 0, not {v['focus_distance']}")
    if not (np.isfinite(v["scale"]) and v["scale"] >= 0.0):
        raise ValueError(f"depth_of_field: scale must be finite and >= 0, not {v['scale']}")
    if not 0.5 <= v["max_radius"] <= _lib.URT_DOF_MAX_RADIUS:
        raise ValueError(f"depth_of_field: max_radius must lie in [0.5, 16], not {v['max_radius']}")
    flags = _int_arg(v["flags"], "flags", "depth_of_field")
    if flags & ~_lib.URT_DOF_FLAG_COC:
        raise ValueError(f"depth_of_field: unknown flag bits in {flags}")
    return _lib.DofParams(v["focus_distance"], v["scale"], v["max_radius"], flags)


def motion_blur_params(**params) -> _lib.MotionBlurParams:
    """The checked urt_MotionBlurParams of Context.motion_blur: shutter finite in [0, 1], max_radius in [0.5, 16], flags 0 or
    _lib.URT_MOTION_BLUR_FLAG_VELOCITY; what is not given is _lib.MOTION_BLUR_DEFAULTS'."""
    unknown = set(params) - set(_lib.MOTION_BLUR_DEFAULTS)
    if unknown:
        raise TypeError(f"motion_blur: unknown parameters {sorted(unknown)}")
    v = {**_lib.MOTION_BLUR_DEFAULTS, **params}
    for name in ("shutter", "max_radius"):
        v[name] = _float32_arg(v[name], name, "motion_blur")
    if not 0.0 <= v["shutter"] <= 1.0:
        raise ValueError(f"motion_blur: shutter must lie in [0, 1], not {v['shutter']}")
    if not 0.5 <= v["max_radius"] <= _lib.URT_MOTION_BLUR_MAX_RADIUS:
        raise ValueError(f"motion_blur: max_radius must lie in [0.5, 16], not {v['max_radius']}")
    flags = _int_arg(v["flags"], "flags", "motion_blur")
    if flags & ~_lib.URT_MOTION_BLUR_FLAG_VELOCITY:
        raise ValueError(f"motion_blur: unknown flag bits in {flags}")
    return _lib.MotionBlurParams(v["shutter"], v["max_radius"], flags, 0)


def dof_scale(height, focus_distance, f_number=5.6, focal_length=0.05, sensor_height=0.024) -> np.float32:
    """urt_DofParams.scale of a physical camera: the thin-lens circle of confusion of a point at infinity as a RADIUS in pixels of an image
    `height` pixels tall, K = 0.5 * height * f^2 / (N * (s - f) * sensor_height), with the lens focused at s = focus_distance, focal
    length f and sensor height in the scene's units (the defaults: Unity's physical camera, 50 mm at f/5.6 on a 24 mm sensor, in metres).
    Evaluated in double precision and rounded once.  s must lie beyond f."""
    h = _int_arg(height, "height", "dof_scale")
    if h <= 0:
        raise ValueError(f"dof_scale: height must be positive, not {h}")
    s, n, f, sh = (_number_arg(v, name, "dof_scale") for name, v in (("focus_distance", focus_distance), ("f_number", f_number),
                                                                       ("focal_length", focal_length), ("sensor_height", sensor_height)))
    for name, v in (("f_number", n), ("focal_length", f), ("sensor_height", sh)):
        if not (np.isfinite(v) and v > 0.0):
            raise ValueError(f"dof_scale: {name} must be finite and > 0, not {v}")
    if not (np.isfinite(s) and s > f):
        raise ValueError(f"dof_scale: focus_distance ({s}) must be finite and lie beyond the focal length ({f})")
    k = np.float32(0.5 * h * f * f / (n * (s - f) * sh))
    if not np.isfinite(k):
        raise ValueError("dof_scale: the scale does not fit a float32")
    return k


def _sync_torch_stream(t):
    """Waits for torch's current stream on the tensor's device: what torch enqueued on it (the tensor's initialisation) is not ordered
    with the library's stream otherwise."""
    import torch
    torch.cuda.current_stream(t.device).synchronize()


# urt_Ray / urt_RayHit (include/urt_types.h) as numpy records
RAY_DT = np.dtype([("origin", np.float32, 3), ("t_max", np.float32), ("direction", np.float32, 3), ("reserved", np.int32)])
RAYHIT_DT = np.dtype([("distance", np.float32), ("position", np.float32, 3), ("normal", np.float32, 3), ("kind", np.int32),
                      ("object", np.int32), ("primitive", np.int32), ("u", np.float32), ("v", np.float32)])


# urt_PathRay / urt_PathPixel (include/urt_types.h) as numpy records
PATHRAY_DT = np.dtype([("origin", np.float32, 3), ("seed", np.float32), ("direction", np.float32, 3), ("reserved0", np.int32),
                       ("px", np.float32), ("py", np.float32), ("reserved1", np.int32, 2)])
PATHPIXEL_DT = np.dtype([("x", np.int32), ("y", np.int32)])

# texels one workgroup of the selection kernels handles (csrc/resample.h kSelectChunk): the sizes at which urt_select_pixels changes path
SELECT_CHUNK = 2048
# workgroups (of 256 lanes) the luminance histogram of urt_auto_exposure launches at most (csrc/tonemap.h kExposureMaxBlocks): an image of
# more texels is grid-strided
EXPOSURE_MAX_BLOCKS = 1024


def _radiance_counts(samples, bounces):
    """The checked (samples, bounces) of Context.radiance_query*: ints in 1..4096 and 0..64 (include/urt.h)."""
    for name, v, lo, hi in (("samples", samples, 1, _lib.RADIANCE_MAX_SAMPLES), ("bounces", bounces, 0, _lib.RADIANCE_MAX_BOUNCES)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"radiance_query: {name} must be an int, not {type(v).__name__}")
        if not lo <= v <= hi:
            raise ValueError(f"radiance_query: {name} must be {lo}..{hi}, not {v}")
    return int(samples), int(bounces)


def _per_ray_arg(v, n: int, name: str, who: str) -> np.ndarray:
    """A number, or a float32 array (n,)."""
    if isinstance(v, np.ndarray):
        if v.dtype != np.float32:
            raise TypeError(f"{who}: {name} must be float32, not {v.dtype}")
        if v.shape != (n,):
            raise ValueError(f"{who}: {name} must be a scalar or have shape ({n},), not {v.shape}")
        return v
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.floating, np.integer)):
        raise TypeError(f"{who}: {name} must be a number or a float32 array, not {type(v).__name__}")
    return np.full(n, v, dtype=np.float32)


def denoise_params(iterations: int = _lib.DENOISE_DEFAULTS["iterations"], sigma_color: float = _lib.DENOISE_DEFAULTS["sigma_color"],
                   sigma_normal: float = _lib.DENOISE_DEFAULTS["sigma_normal"],
                   sigma_depth: float = _lib.DENOISE_DEFAULTS["sigma_depth"]) -> _lib.DenoiseParams:
    """The checked urt_DenoiseParams of Context.denoise: iterations an int in 1..5, each sigma a number that is not NaN."""
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)):
        raise TypeError(f"denoise: iterations must be an int, not {type(iterations).__name__}")
    if not 1 <= iterations <= 5:
        raise ValueError(f"denoise: iterations must be 1..5, not {iterations}")
    sigmas = {"sigma_color": sigma_color, "sigma_normal": sigma_normal, "sigma_depth": sigma_depth}
    for name, v in sigmas.items():
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError(f"denoise: {name} must be a number, not {type(v).__name__}")
        if np.isnan(v):
            raise ValueError(f"denoise: {name} is NaN")
    return _lib.DenoiseParams(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_depth))


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


def _rays_arg(a, name: str, who: str = "ray_query") -> np.ndarray:
    if not isinstance(a, np.ndarray):
        raise TypeError(f"{who}: {name} must be a numpy array (or a torch tensor), not {type(a).__name__}")
    if a.dtype != np.float32:
        raise TypeError(f"{who}: {name} must be float32, not {a.dtype}")
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"{who}: {name} must have shape (n, 3), not {a.shape}")
    if a.shape[0] > 0x7fffffff:
        raise ValueError(f"{who}: more than 2^31 - 1 rays")
    return a


def _t_max_arg(t_max, n: int) -> np.ndarray:
    if t_max is None:
        return np.full(n, np.inf, dtype=np.float32)
    if isinstance(t_max, np.ndarray):
        if t_max.dtype != np.float32:
            raise TypeError(f"ray_query: t_max must be float32, not {t_max.dtype}")
        if t_max.shape != (n,):
            raise ValueError(f"ray_query: t_max must be a scalar or have shape ({n},), not {t_max.shape}")
        return t_max
    if not isinstance(t_max, (int, float, np.floating, np.integer)):
        raise TypeError(f"ray_query: t_max must be a number or a float32 array, not {type(t_max).__name__}")
    return np.full(n, t_max, dtype=np.float32)


class _GroupLib:
    """Maps the per-context entry points onto their urt_group_* counterparts, so that ComputeBuffer / RenderTexture /
    ComputeShader / Graphics / RayTraceMaster drive a DeviceGroup exactly as they drive a Context."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if not name.startswith("urt_"):
            raise AttributeError(name)
        return getattr(self._lib, "urt_group_" + name[4:])       # AttributeError for calls a group does not offer


class DeviceGroup:
    """urt_group: ONE host thread drives N GPUs (include/urt.h "device groups").  Scene, uniforms, textures and blits are
    replicated on every rank, Dispatch is partitioned into 8-row strips with global pixel ids, `gather` is the one exchange
    per frame (strips -> full image on rank 0).  `devices` may repeat an ordinal (several ranks on one card)."""

    def __init__(self, devices):
        self._raw = _lib.load()
        self.lib = _GroupLib(self._raw)
        self._h = C.c_void_p()
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        rc = self._raw.urt_group_create(arr, len(devices), C.byref(self._h))
        if rc != 0:
            raise UrtError(rc, self._raw.urt_group_last_error(None).decode())
        self.devices = list(devices)

    @property
    def size(self) -> int:
        return self._raw.urt_group_size(self._h)

    def check(self, rc: int):
        if rc != 0:
            raise UrtError(rc, self._raw.urt_group_last_error(self._h).decode())

    def close(self):
        if self._h:
            self._raw.urt_group_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def synchronize(self):
        self.check(self._raw.urt_group_synchronize(self._h))

    def flush(self):
        self.check(self._raw.urt_group_flush(self._h))

    def set_option(self, name: str, value: int):
        self.check(self._raw.urt_group_set_option(self._h, name.encode(), int(value)))

    def gather(self, src: "RenderTexture", dst: "RenderTexture"):
        """The ONE exchange per frame: every rank's strips of `src` -> the full image `dst` on rank 0."""
        self.check(self._raw.urt_group_gather(self._h, src.handle, dst.handle))

    def counters(self) -> dict:
        c = Counters()
        self.check(self._raw.urt_group_get_counters(self._h, C.byref(c)))
        return c.as_dict()

    def reset_counters(self):
        self.check(self._raw.urt_group_reset_counters(self._h))


class ComputeBuffer:
    """UnityEngine.ComputeBuffer (RM:247-250)."""

    def __init__(self, ctx: Context, count: int, stride: int):
        self.ctx = ctx
        h = C.c_uint64()
        ctx.check(ctx.lib.urt_buffer_create(ctx._h, int(count), int(stride), C.byref(h)))
        self.handle = h.value
        self.count, self.stride = int(count), int(stride)

    def SetData(self, data, managed_start: int = 0, compute_start: int = 0, count: int | None = None):
        """SetData(data): the whole list.  SetData(data, managed_start, compute_start, count): Unity's ranged overload — `count` elements
        of `data` from element managed_start on go to elements compute_start .. compute_start + count - 1 of the buffer
        (include/urt.h urt_buffer_set_data_range)."""
        a = np.ascontiguousarray(data)
        if a.nbytes % self.stride:
            raise UrtError(1, f"SetData: {a.nbytes} bytes is not a multiple of stride {self.stride}")
        n = a.nbytes // self.stride
        if managed_start == 0 and compute_start == 0 and count is None:
            self.ctx.check(self.ctx.lib.urt_buffer_set_data(self.ctx._h, self.handle, a.ctypes.data_as(C.c_void_p), n))
            return
        for name, v in (("managed_start", managed_start), ("compute_start", compute_start), ("count", n if count is None else count)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"SetData: {name} must be an int, not {type(v).__name__}")
        count = n - managed_start if count is None else count
        if managed_start < 0 or count < 0 or managed_start + count > n:
            raise UrtError(1, f"SetData: elements {managed_start} .. {managed_start + count - 1} lie outside the {n} elements of data")
        ptr = C.c_void_p(a.ctypes.data + int(managed_start) * self.stride) if n else C.c_void_p(0)
        self.ctx.check(self.ctx.lib.urt_buffer_set_data_range(self.ctx._h, self.handle, int(compute_start), ptr, int(count)))

    def SetDataDevice(self, tensor_or_ptr, compute_start: int = 0, count: int | None = None):
        """Ranged SetData from DEVICE memory (include/urt.h urt_buffer_set_data_device): `count` elements go to elements compute_start ..
        compute_start + count - 1 of the buffer.  A contiguous torch tensor on the context's device (count defaults to what it holds; what
        torch's current stream has written to it is waited for first), or a raw device address with an explicit count, whose producer the
        caller orders.  The copy is enqueued on the context's stream and not waited for: the source stays as it is until
        ctx.synchronize()."""
        for name, v in (("compute_start", compute_start), ("count", 0 if count is None else count)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"SetDataDevice: {name} must be an int, not {type(v).__name__}")
        if _is_torch(tensor_or_ptr):
            import torch
            t = tensor_or_ptr
            if t.device.type != "cuda" or t.device.index != self.ctx.device:
                raise ValueError(f"SetDataDevice: the tensor must be on cuda:{self.ctx.device}, not {t.device}")
            if not t.is_contiguous():
                raise ValueError("SetDataDevice: the tensor must be contiguous")
            nbytes = t.numel() * t.element_size()
            if nbytes % self.stride:
                raise UrtError(1, f"SetDataDevice: {nbytes} bytes is not a multiple of stride {self.stride}")
            count = nbytes // self.stride if count is None else count
            if count < 0 or count * self.stride > nbytes:
                raise UrtError(1, f"SetDataDevice: {count} elements lie outside the {nbytes // self.stride} elements of the tensor")
            torch.cuda.current_stream(t.device).synchronize()
            ptr = t.data_ptr() if nbytes else 0
        else:
            if isinstance(tensor_or_ptr, (bool, np.bool_)) or not isinstance(tensor_or_ptr, (int, np.integer)):
                raise TypeError(f"SetDataDevice: a torch tensor or a device address is needed, not {type(tensor_or_ptr).__name__}")
            if count is None:
                raise TypeError("SetDataDevice: count is needed with a device address")
            ptr = int(tensor_or_ptr)
        self.ctx.check(self.ctx.lib.urt_buffer_set_data_device(self.ctx._h, self.handle, int(compute_start), C.c_void_p(ptr), int(count)))

    def CopyFrom(self, src: "ComputeBuffer", src_first: int = 0, dst_first: int = 0, count: int | None = None):
        """A snapshot on the device (include/urt.h urt_buffer_copy): `count` elements of src from src_first on go to elements dst_first ..
        dst_first + count - 1 of this buffer, mirror to mirror on the context's stream: nothing is downloaded or waited for.  count
        defaults to what src holds from src_first on."""
        if not isinstance(src, ComputeBuffer):
            raise TypeError(f"CopyFrom: src must be a ComputeBuffer, not {type(src).__name__}")
        if src.ctx is not self.ctx:
            raise ValueError("CopyFrom: src belongs to another context")
        for name, v in (("src_first", src_first), ("dst_first", dst_first), ("count", 0 if count is None else count)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"CopyFrom: {name} must be an int, not {type(v).__name__}")
        count = src.count - int(src_first) if count is None else count
        self.ctx.check(self.ctx.lib.urt_buffer_copy(self.ctx._h, src.handle, int(src_first), self.handle, int(dst_first), int(count)))

    def GetData(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """ComputeBuffer.GetData: elements first .. first + count - 1 as the buffer holds them now, as (count, stride) bytes — the caller
        views them as its element type (include/urt.h urt_buffer_get_data_range; downloads what was written on the device, waits)."""
        count = self.count - int(first) if count is None else count
        out = np.zeros((max(0, int(count)), self.stride), dtype=np.uint8)
        self.ctx.check(self.ctx.lib.urt_buffer_get_data_range(self.ctx._h, self.handle, int(first), out.ctypes.data_as(C.c_void_p), int(count)))
        return out

    def Release(self):
        if self.handle:
            self.ctx.check(self.ctx.lib.urt_buffer_release(self.ctx._h, self.handle))
            self.handle = 0


class NormalsPlan:
    """RayTraceMaster.ComputeNormals on the GPU for one vertex span (include/urt.h, "normals on the device"): made once per topology from
    the buffers' contents at that time, then .compute(dst_normals) recomputes the span's normals from the CURRENT device-side positions
    into the device side of dst_normals — two kernels on the context's stream, nothing waited for, nothing downloaded.  The result is
    urt_host_compute_normals of the current positions whenever they weld as the plan-time positions did."""

    def __init__(self, ctx: Context, vertices: "ComputeBuffer", indices: "ComputeBuffer", first: int = 0, count: int | None = None):
        for name, b in (("vertices", vertices), ("indices", indices)):
            if not isinstance(b, ComputeBuffer):
                raise TypeError(f"normals_plan: {name} must be a ComputeBuffer, not {type(b).__name__}")
            if b.ctx is not ctx:
                raise ValueError(f"normals_plan: {name} belongs to another context")
        for name, v in (("first", first), ("count", 0 if count is None else count)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"normals_plan: {name} must be an int, not {type(v).__name__}")
        count = vertices.count - int(first) if count is None else count
        self.ctx, self.handle = ctx, 0
        h = C.c_uint64()
        ctx.check(ctx.lib.urt_normals_plan_create(ctx._h, vertices.handle, indices.handle, int(first), int(count), C.byref(h)))
        self.handle = h.value

    @property
    def info(self) -> dict:
        """first, count, n_lists, n_triangles, n_entries, max_valence, device_bytes (include/urt.h urt_NormalsPlanInfo)."""
        a = _lib.NormalsPlanInfo()
        self.ctx.check(self.ctx.lib.urt_normals_plan_info(self.ctx._h, self.handle, C.byref(a)))
        return {n: int(getattr(a, n)) for n, _ in _lib.NormalsPlanInfo._fields_}

    def compute(self, dst_normals: "ComputeBuffer"):
        if not isinstance(dst_normals, ComputeBuffer):
            raise TypeError(f"NormalsPlan.compute: dst_normals must be a ComputeBuffer, not {type(dst_normals).__name__}")
        self.ctx.check(self.ctx.lib.urt_compute_normals(self.ctx._h, self.handle, dst_normals.handle))

    def Release(self):
        if self.handle:
            self.ctx.check(self.ctx.lib.urt_normals_plan_release(self.ctx._h, self.handle))
            self.handle = 0


class MorphPlan:
    """Blend shapes (morph targets) on the GPU for one vertex span (include/urt.h, "blend shapes on the device"): the deltas of every
    target laid out per served vertex, made once per mesh; .morph(...) adds them, scaled by the weight table, to a rest pose into the
    device side of the destinations — one kernel on the context's stream, nothing waited for, nothing downloaded."""

    def __init__(self, ctx: Context, deltas, n_targets: int, first: int, count: int):
        from . import host_scene
        for name, v in (("n_targets", n_targets), ("first", first), ("count", count)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"morph_plan: {name} must be an int, not {type(v).__name__}")
        try:
            d = host_scene.morph_deltas(deltas)
        except (TypeError, ValueError):
            raise ValueError("morph_plan: deltas must be an array of urt_MorphDelta or a sequence of (vertex, target, dp[3], dn[3])") from None
        self.ctx, self.handle = ctx, 0
        h = C.c_uint64()
        ctx.check(ctx.lib.urt_morph_plan_create(ctx._h, d.ctypes.data_as(C.c_void_p) if d.size else None, len(d), int(n_targets), int(first),
                                                int(count), C.byref(h)))
        self.handle = h.value

    def info(self) -> dict:
        """first, count, n_targets, n_entries, max_valence, n_touched, device_bytes (include/urt.h urt_MorphPlanInfo)."""
        a = _lib.MorphPlanInfo()
        self.ctx.check(self.ctx.lib.urt_morph_plan_info(self.ctx._h, self.handle, C.byref(a)))
        return {n: int(getattr(a, n)) for n, _ in _lib.MorphPlanInfo._fields_}

    def morph(self, rest_v, rest_n, weights, dst_v, dst_n, normalize: bool = False):
        """dst_v (and dst_n) [first .. first + count - 1] = rest_v (rest_n) + the weighted deltas (urt_morph_vertices).  rest_v, dst_v,
        rest_n, dst_n: stride-12 ComputeBuffers of one count; rest_n and dst_n may be None (positions only).  weights: a stride-4
        ComputeBuffer of n_targets floats.  normalize: URT_MORPH_NORMALIZE."""
        handle = functools.partial(_buffer_handle, self.ctx, "MorphPlan.morph")
        self.ctx.check(self.ctx.lib.urt_morph_vertices(self.ctx._h, self.handle, handle(rest_v, "rest_v"), handle(rest_n, "rest_n", True),
                                                       handle(weights, "weights"), handle(dst_v, "dst_v"), handle(dst_n, "dst_n", True),
                                                       _lib.MORPH_NORMALIZE if normalize else 0))

    def Release(self):
        if self.handle:
            self.ctx.check(self.ctx.lib.urt_morph_plan_release(self.ctx._h, self.handle))
            self.handle = 0


class RenderTexture:
    """UnityEngine.RenderTexture(w, h, 0, ARGBFloat, Linear) with enableRandomWrite (RM:834-840).
    Row 0 is the bottom row.  `external_ptr` wraps caller-owned device memory (e.g. a torch tensor)."""

    def __init__(self, ctx: Context, width: int, height: int, external_ptr: int | None = None):
        self.ctx = ctx
        h = C.c_uint64()
        if external_ptr is None:
            ctx.check(ctx.lib.urt_texture_create(ctx._h, int(width), int(height), C.byref(h)))
        else:
            ctx.check(ctx.lib.urt_texture_create_external(ctx._h, int(width), int(height), C.c_void_p(external_ptr), C.byref(h)))
        self.handle = h.value
        self.width, self.height = int(width), int(height)

    def Release(self):
        if self.handle:
            self.ctx.check(self.ctx.lib.urt_texture_release(self.ctx._h, self.handle))
            self.handle = 0

    def SetPixels(self, rgba):
        a = np.ascontiguousarray(rgba, dtype=np.float32)
        if a.size != self.width * self.height * 4:
            raise UrtError(1, "SetPixels: expected height*width*4 floats")
        self.ctx.check(self.ctx.lib.urt_texture_set_pixels(self.ctx._h, self.handle, a.ctypes.data_as(C.c_void_p)))

    def GetPixels(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self.ctx.check(self.ctx.lib.urt_texture_get_pixels(self.ctx._h, self.handle, out.ctypes.data_as(C.c_void_p)))
        return out

    FORMATS = {"RGBA32F": (0, np.float32), "RGBA8_SRGB": (1, np.uint8), "RGBA16F": (2, np.float16)}   # include/urt.h URT_FORMAT_*

    def ReadBegin(self, format: str = "RGBA32F") -> int:
        """Start a pipelined readback of the image as it is now (include/urt.h urt_texture_read_begin_format), converted on the GPU to
        `format` ("RGBA32F", "RGBA8_SRGB": what an 8-bit back buffer holds after RM:819, "RGBA16F"); returns a ticket."""
        t = C.c_uint64()
        self.ctx.check(self.ctx.lib.urt_texture_read_begin_format(self.ctx._h, self.handle, self.FORMATS[format][0], C.byref(t)))
        self._read_formats = getattr(self, "_read_formats", {})
        self._read_formats[t.value] = format
        return t.value

    def ReadEnd(self, ticket: int, copy: bool = True) -> np.ndarray:
        """Wait for that readback; the image as (height, width, 4) of the ticket's format — a copy, or (copy=False) a view of the
        library's pinned buffer that stays valid until the third ReadBegin after the ticket's."""
        dtype = self.FORMATS[getattr(self, "_read_formats", {}).pop(ticket, "RGBA32F")][1]
        p, n = C.c_void_p(), C.c_size_t()
        self.ctx.check(self.ctx.lib.urt_texture_read_end_format(self.ctx._h, C.c_uint64(ticket), C.byref(p), C.byref(n)))
        assert n.value == self.height * self.width * 4 * np.dtype(dtype).itemsize
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,)).view(dtype).reshape(self.height, self.width, 4)
        return a.copy() if copy else a

    def device_ptr(self) -> int:
        p = C.c_void_p()
        self.ctx.check(self.ctx.lib.urt_texture_get_info(self.ctx._h, self.handle, None, None, C.byref(p)))
        return p.value

    def packed_bytes(self, first_group_row: int, row_stride: int) -> int:
        n = C.c_uint64()
        self.ctx.check(self.ctx.lib.urt_texture_pack_rows(self.ctx._h, self.handle, first_group_row, row_stride, None, C.byref(n)))
        return n.value

    def pack_rows(self, first_group_row: int, row_stride: int, device_dst: int, rgb: bool = False):
        """This rank's strips -> a dense device buffer; rgb: three channels per pixel (include/urt.h urt_texture_pack_rows_rgb)."""
        fn = self.ctx.lib.urt_texture_pack_rows_rgb if rgb else self.ctx.lib.urt_texture_pack_rows
        self.ctx.check(fn(self.ctx._h, self.handle, first_group_row, row_stride, C.c_void_p(device_dst), None))

    def unpack_rows_rgb(self, first_group_row: int, row_stride: int, device_src: int, alpha: float, stream: int | None = None):
        """De-interleave RGB strips into this image, writing `alpha` (running_mean_alpha) into the fourth channel."""
        self.ctx.check(self.ctx.lib.urt_texture_unpack_rows_rgb(self.ctx._h, self.handle, first_group_row, row_stride, C.c_void_p(device_src),
                                                                float(alpha), C.c_void_p(stream or 0)))

    def unpack_rows(self, first_group_row: int, row_stride: int, device_src: int, stream: int | None = None):
        """De-interleave packed strips into this image; `stream` = a caller-ordered hipStream_t (include/urt.h
        urt_texture_unpack_rows_on), default = the context's stream."""
        if stream:
            self.ctx.check(self.ctx.lib.urt_texture_unpack_rows_on(self.ctx._h, self.handle, first_group_row, row_stride, C.c_void_p(device_src), C.c_void_p(stream)))
        else:
            self.ctx.check(self.ctx.lib.urt_texture_unpack_rows(self.ctx._h, self.handle, first_group_row, row_stride, C.c_void_p(device_src)))


Texture2D = RenderTexture   # the sky is an ordinary RGBA32F image here


import struct as _struct
_PACK4 = _struct.Struct("4f").pack


class ComputeShader:
    """UnityEngine.ComputeShader for RayTraceShader.compute; kernel 0 is CSMain."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._bound = ctx.__dict__.setdefault("_bound", {})   # what this context last received, per name (shared by every wrapper of the context)

    def FindKernel(self, name: str) -> int:
        if name != "CSMain":
            raise UrtError(1, f"FindKernel: no kernel named {name}")
        return 0

    # The reference re-sets every uniform and binding every frame (RM:772-795).  Setting a name to the value it already has is
    # a no-op at the boundary, so the wrapper remembers what this context last received per name and skips the call: the host
    # loop of a frame drops from ~18 to ~9 us, which is GPU idle time before a batch of deferred frames is submitted.
    def SetMatrix(self, name: str, m16):
        a = np.ascontiguousarray(m16, dtype=np.float32).reshape(16)
        key, val = ("m", name), a.tobytes()
        if self._bound.get(key) == val:
            return
        self.ctx.check(self.ctx.lib.urt_shader_set_matrix(self.ctx._h, name.encode(), a.ctypes.data_as(C.c_void_p)))
        self._bound[key] = val                                 # only what the library accepted

    def SetVector(self, name: str, v):
        # (the per-frame _PixelOffset: packed with struct, not numpy — 3 us -> 0.6 us of the host's 9 us per frame)
        n = len(v)
        val = _PACK4(float(v[0]) if n > 0 else 0.0, float(v[1]) if n > 1 else 0.0, float(v[2]) if n > 2 else 0.0, float(v[3]) if n > 3 else 0.0)
        key = ("v", name)
        if self._bound.get(key) == val:
            return
        self.ctx.check(self.ctx.lib.urt_shader_set_vector(self.ctx._h, name.encode(), val))
        self._bound[key] = val

    def SetFloat(self, name: str, v: float):
        key, val = ("f", name), C.c_float(v).value             # the float32 the library will see
        if self._bound.get(key) == val and val == val:
            return
        self.ctx.check(self.ctx.lib.urt_shader_set_float(self.ctx._h, name.encode(), float(v)))
        self._bound[key] = val

    def SetInt(self, name: str, v: int):
        key, val = ("i", name), int(v)
        if self._bound.get(key) == val:
            return
        self.ctx.check(self.ctx.lib.urt_shader_set_int(self.ctx._h, name.encode(), val))
        self._bound[key] = val
        self._bound["owner"] = None                             # (a RayTraceMaster's "nothing changed" shortcut ends: ray_trace_master.SetShaderParameters)

    def SetTexture(self, kernel: int, name: str, tex: RenderTexture | None):
        key, h = ("t", kernel, name), tex.handle if tex else 0
        if self._bound.get(key) == h:
            return
        self.ctx.check(self.ctx.lib.urt_shader_set_texture(self.ctx._h, kernel, name.encode(), h))
        self._bound[key] = h

    def SetBuffer(self, kernel: int, name: str, buf: ComputeBuffer | None):
        key, h = ("b", kernel, name), buf.handle if buf else 0
        if self._bound.get(key) == h:
            return
        self.ctx.check(self.ctx.lib.urt_shader_set_buffer(self.ctx._h, kernel, name.encode(), h))
        self._bound[key] = h
        self._bound["owner"] = None

    def Dispatch(self, kernel: int, groups_x: int, groups_y: int, groups_z: int):
        self.ctx.check(self.ctx.lib.urt_shader_dispatch(self.ctx._h, kernel, groups_x, groups_y, groups_z))

    def DispatchRows(self, kernel: int, groups_x: int, groups_y: int, groups_z: int, first_group_row: int, row_stride: int):
        """Multi-GPU extension: only the 8-row strips first_group_row, +row_stride, ... (global pixel ids kept)."""
        self.ctx.check(self.ctx.lib.urt_shader_dispatch_rows(self.ctx._h, kernel, groups_x, groups_y, groups_z, first_group_row, row_stride))


class Material:
    """new Material(Shader.Find("Hidden/AdditionShader")) (RM:813-815)."""

    def __init__(self, shader_name: str = "Hidden/AdditionShader"):
        if shader_name != "Hidden/AdditionShader":
            raise UrtError(1, f"Shader.Find: {shader_name} not found")
        self.floats = {"_Sample": 0.0}

    def SetFloat(self, name: str, v: float):
        self.floats[name] = float(v)


class Graphics:
    @staticmethod
    def Blit(source: RenderTexture, dest: RenderTexture, mat: Material | None = None):
        """Graphics.Blit(src, dst[, additionMaterial]) — RM:818-819."""
        ctx = source.ctx
        if mat is None:
            ctx.check(ctx.lib.urt_blit(ctx._h, source.handle, dest.handle))
        else:
            ctx.check(ctx.lib.urt_blit_add(ctx._h, source.handle, dest.handle, mat.floats["_Sample"]))


def live_resources() -> dict:
    """What the library holds right now, process-wide (urt_debug_live_resources): device bytes, pinned host bytes, events, streams."""
    lib = _lib.load()
    out = (C.c_uint64 * 4)()
    rc = lib.urt_debug_live_resources(out)
    if rc != 0:
        raise UrtError(rc, lib.urt_last_error(None).decode())
    return dict(zip(("device_bytes", "pinned_bytes", "events", "streams"), (int(v) for v in out)))


def debug_build_blas(mesh_objects: np.ndarray, vertices: np.ndarray, indices: np.ndarray):
    """Run the library's triangle-BVH builder on host arrays (no GPU needed) and return
    (nodes[n,16] f32, tri_index[n_tris] i32, mesh_root[n_meshes] i32, mesh_first_tri, max_depth)."""
    lib = _lib.load()
    mo = np.ascontiguousarray(mesh_objects)
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    ix = np.ascontiguousarray(indices, dtype=np.int32)
    nn, nt, md = C.c_int(), C.c_int(), C.c_int()
    rc = lib.urt_debug_build_blas(mo.ctypes.data_as(C.c_void_p), len(mo), v.ctypes.data_as(C.c_void_p), len(v.reshape(-1, 3)),
                                  ix.ctypes.data_as(C.c_void_p), ix.size, C.byref(nn), C.byref(nt), C.byref(md))
    if rc != 0:
        raise UrtError(rc, lib.urt_last_error(None).decode())
    nodes = np.zeros((nn.value, 16), dtype=np.float32)
    tri = np.zeros(nt.value, dtype=np.int32)
    root = np.zeros(len(mo), dtype=np.int32)
    first = np.zeros(len(mo), dtype=np.int32)
    lib.urt_debug_get_blas(nodes.ctypes.data_as(C.c_void_p), tri.ctypes.data_as(C.c_void_p), root.ctypes.data_as(C.c_void_p),
                           first.ctypes.data_as(C.c_void_p))
    return nodes, tri, root, first, md.value
