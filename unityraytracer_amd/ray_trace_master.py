"""Host-side mirror of Assets/Scripts/RayTraceMaster.cs — the frame driver around the hot path.

Method names and order of GPU calls follow the reference (RM = RayTraceMaster.cs):

    OnRenderImage (RM:848-866)  ->  [RebuildTrees (RM:725-746)]  ->  SetShaderParameters (RM:772-795)
                                ->  Render (RM:798-821)  ->  InitRenderTexture (RM:824-845)

The scene arrives already flattened (a `scenes.Scene`: what RebuildObjectLists RM:262-336 and the BVH
builder RM:405-722 produce); `RebuildTrees` here is the upload half of the reference's: the seven
CreateComputeBuffer calls (RM:738-745).  `UnityEngine.Random.value` (RM:777-778) is replaced by the
documented splitmix64 frame sequence of scenes.frame_uniforms so that frames are reproducible.

Multi-GPU (one process per GPU): construct with rank/world_size; each rank renders the 8-row strips
rank, rank+world, ... with GLOBAL pixel ids and accumulates locally; `gather_converged` moves the
strips to rank 0 with one collective at frame end.
"""
from __future__ import annotations

import math

import numpy as np

from dataclasses import dataclass, field

from . import _lib, host_scene, scenes
from .unity_api import ComputeBuffer, ComputeShader, Context, Graphics, Material, RenderTexture, _matrix16, _max_history_arg, \
    _number_arg, denoise_params, reproject_params


@dataclass
class RayTraceObject:
    """Assets/Scripts/RayTraceObject.cs: what a scene object contributes (RO:9-19).  type 1 = analytic sphere
    (position, radius), anything else = mesh (vertices, triangles of submesh 0, localToWorldMatrix)."""
    type: int = 0
    albedoColor: tuple = (0.0, 0.4, 1.0)          # RO:12
    specularColor: tuple = (0.7, 0.0, 1.0)        # RO:13
    emissionColor: tuple = (0.0, 0.0, 0.0)        # RO:14
    smoothness: float = 0.69                      # RO:15
    position: tuple = (0.0, 0.0, 0.0)             # RO:34 (spheres)
    radius: float = 0.5                           # RO:33 (spheres)
    vertices: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), np.float32))      # mesh.vertices
    triangles: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), np.int32))       # mesh.GetIndices(0)
    localToWorldMatrix: np.ndarray = field(default_factory=lambda: scenes.trs())            # transform.localToWorldMatrix


def _index_arg(k, n: int, who: str, what: str, names: str):
    """k names one of the scene's n objects, or the error the edits raise: `what` is what must be ints, `names` how k is quoted."""
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"{who}: {what} must be ints, not {type(k).__name__}")
    if not 0 <= k < n:
        raise IndexError(f"{who}: {names} {k}, the scene has {n}")


def _device_list_arg(a, stride: int, name: str):
    """A list in device memory for ReplaceGeometryDevice: a torch tensor, or (device address, element count) -> (what
    ComputeBuffer.SetDataDevice takes, element count)."""
    if isinstance(a, tuple) and len(a) == 2:
        ptr, count = a
        for what, v in (("device address", ptr), ("count", count)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"ReplaceGeometryDevice: the {what} of {name} must be an int, not {type(v).__name__}")
        if count < 0:
            raise ValueError(f"ReplaceGeometryDevice: the count of {name} is negative")
        return int(ptr), int(count)
    if hasattr(a, "data_ptr") and hasattr(a, "element_size"):
        nbytes = a.numel() * a.element_size()
        if nbytes % stride:
            raise ValueError(f"ReplaceGeometryDevice: {name} holds {nbytes} bytes, not a multiple of its stride {stride}")
        return a, nbytes // stride
    raise TypeError(f"ReplaceGeometryDevice: {name} must be a torch tensor or (device address, count), not {type(a).__name__}")


class RayTraceMaster:
    MeshObjectStructSize = 112   # RM:43
    SphereStructSize = 56        # RM:44
    BVHNodeSize = 28             # RM:45
    _normalsPlans = {}           # (the instance's own from __init__ on; here so that host-only use of a master made without one has none to drop)

    _uplow = _upaov = _upcount = _upscaled = _uptarget = None   # (likewise: Upscale's textures)
    _exposure = _exposureState = _tonemapped = None             # (likewise: auto-exposure and ToneMap)
    _bloom = None                                               # (likewise: EnableBloom)
    _dof = _dofHit = None                                       # (likewise: EnableDepthOfField)
    _mblur = _mbMotion = _mbStage = _mbAge = None               # (likewise: EnableMotionBlur)
    # With True, SkinMeshes, MorphMeshes and MoveObjects build the object-level heaps on the GPU (include/urt.h "the object-level BVH on the
    # device": urt_mesh_leaf_bounds_device / urt_sphere_leaf_bounds_device, then urt_build_object_bvh_device into the heap buffers) instead
    # of on the host, and make no synchronising call of their own.  scene.mesh_bvh / scene.sphere_bvh are then BEHIND the device, as
    # scene.vertices already is after SkinMeshes: a host that wants them (OnDrawGizmos, a checkpoint of the scene) calls SyncObjectHeaps()
    # first, which reads them back (GetData: it synchronises).  The boxes are those of the host functions (the mesh's own points), not the
    # loose box of eight transformed corners.  False (the default): nothing differs from a master without the attribute.
    device_object_heaps = False
    # device_prepare (a property, below): with True the context's full preparations take _Vertices / _Indices / _Normals from the buffers'
    # device side (include/urt.h option "prepare_device").  False (the default): nothing differs from a master without the attribute.
    _devicePrepare = False
    _geometryBehind = False                                     # (ReplaceGeometryDevice: scene.vertices / indices / normals are behind their buffers)
    _leafBuffers = (None, None)                                 # (likewise: the leaf records the device heaps are built from)
    _heapsBehind = (False, False)                               # (likewise: scene.mesh_bvh / scene.sphere_bvh are behind their buffers)

    def __init__(self, ctx: Context, scene: scenes.Scene, rank: int = 0, world_size: int = 1, frame_seed: int = 0x5EED):
        self.ctx = ctx
        self.RayTraceShader = ComputeShader(ctx)
        self.scene = scene
        self.numBounces = scene.num_bounces          # RM:17
        self.numRays = scene.num_rays                # RM:18
        self.rank, self.world_size = rank, world_size
        self.frame_seed = frame_seed
        self._currentSample = 0                      # RM:19
        self._bindings_key = None                    # what SetShaderParameters last bound (its every-frame re-set is skipped while nothing changed)
        self._frame = 0
        self._target = None                          # RM:11
        self._converged = None                       # RM:12
        self._additionMaterial = None                # RM:20
        self._treesNeedRebuilding = True             # RM:24
        self._rayTraceObjects = []                   # RM:22 (empty: the scene arrives pre-flattened in `scene`)
        self.SkyboxTexture = None                    # RM:10
        self.rayDebug = None                         # RM:9: a RayTraceDebug (ray_trace_debug.py) or None
        self._meshObjectBuffer = self._vertexBuffer = self._indexBuffer = self._normalBuffer = None
        self._sphereBuffer = self._meshObjectBVHBuffer = self._sphereBVHBuffer = None
        self.screen_width, self.screen_height = scene.width, scene.height
        self._aov = None                             # RenderFeatureBuffers: (hit, normal, albedo, id) of the screen size
        self._denoised = None                        # Denoise without a destination: the denoised image
        self._uplow = self._upaov = None             # Upscale: (hit, normal, albedo, id) of the traced and of the presented size, through the sample centres
        self._upcount = self._upscaled = self._uptarget = None   # Upscale: the count texture, the image (without a destination), fill_holes' Result
        self.upscaleFilled = 0                       # Upscale(fill_holes=True): the pixels the last call traced at full resolution
        self._exposure = None                        # EnableAutoExposure: the urt_ExposureParams fields given (None = off)
        self._exposureState = None                   # EnableAutoExposure: the urt_ExposureState, a torch tensor on the context's device
        self._tonemapped = None                      # ToneMap without a destination: the tone-mapped image
        self._bloom = None                           # EnableBloom: the urt_BloomParams fields given (None = off)
        self._dof = None                             # EnableDepthOfField: the urt_DofParams fields given (None = off)
        self._dofHit = None                          # ToneMap with depth of field on: the hit guide of _converged's size
        self._mblur = None                           # EnableMotionBlur: the urt_MotionBlurParams fields given (None = off)
        self._mbMotion = None                        # motion blur: the motion image the edits' reprojection writes, of _converged's size
        self._mbStage = None                         # ToneMap with depth of field AND motion blur on: the image between the two
        self._mbAge = None                           # motion blur: frames rendered since _mbMotion was written (None = it holds nothing)
        self._temporal = None                        # EnableTemporalAccumulation: the reprojection settings (None = off, the reference's behaviour)
        self._tcount = self._tspare = None           # temporal: the count texture of _converged; the spare (colour, count) pair reprojection writes
        self._taov = None                            # temporal: two (hit, normal, id) sets, the previous and the new camera's
        self._moved_max_history = 0.0                # temporal: extra clamp of the count on pixels of moved objects (MoveObjects; 0 = none)
        self._tmotion = [None, None]                 # temporal: the mesh and the sphere motion table of the last MoveObjects (ComputeBuffers)
        self._tdeform = [None, None, None]           # temporal, keep_history: previous positions, previous _MeshObjects, per-mesh flags (ComputeBuffers)
        self._deform_normal_threshold = None         # temporal, keep_history: urt_ReprojectDeform.normal_threshold (None = the library's default)
        self._skins = {}                             # AttachSkin: MeshObject index -> its span, rest pose, bone indices and weights
        self._skinBuffers = None                     # SkinMeshes: rest vertices, rest normals, bone indices, bone weights (ComputeBuffers of the vertex count)
        self._boneBuffers = {}                       # SkinMeshes: MeshObject index -> its bone table (ComputeBuffer)
        self._skinBoxes = {}                         # SkinMeshes: MeshObject index -> object-space (min, max) of its skinned span, from the GPU
        self._boxCache = {}                          # SkinMeshes: MeshObject index -> (matrix bytes, id of the vertex list, world lo, world hi)
        self._morphs = {}                            # AttachBlendShapes: MeshObject index -> its span, rest pose, deltas, target count and (from the first MorphMeshes on) MorphPlan
        self._morphBuffers = None                    # MorphMeshes: rest vertices, rest normals, and the pair a morph ahead of a skin writes into (ComputeBuffers of the vertex count)
        self._morphWeightBuffers = {}                # MorphMeshes: MeshObject index -> its weight table (ComputeBuffer)
        self._leafBuffers = [None, None]             # device_object_heaps: the mesh and the sphere leaf records (ComputeBuffers of the object counts)
        self._heapsBehind = [False, False]           # device_object_heaps: scene.mesh_bvh / scene.sphere_bvh are behind the heap buffers' device side
        self._normalsPlans = {}                      # RecomputeNormals: MeshObject index -> ((vertex buffer, index buffer, first, last), NormalsPlan, the index list it was made for)

    # Geometry that ReplaceGeometryDevice, SkinMeshes, MorphMeshes or SetDataDevice wrote on the device is then never downloaded for a
    # rebuild (new topology, buffers of another count, a rebuild forced by "refit_rebuild_pct"), and the triangle BVHs are always built
    # on the GPU.  Setting it sets the context's option, which every master of the context shares.
    @property
    def device_prepare(self) -> bool:
        return self._devicePrepare

    @device_prepare.setter
    def device_prepare(self, on):
        self.ctx.set_option("prepare_device", 1 if on else 0)
        self._devicePrepare = bool(on)

    # RM:215-230
    def RegisterObject(self, obj: RayTraceObject):
        self._rayTraceObjects.append(obj)
        self._treesNeedRebuilding = True

    def UnregisterObject(self, obj: RayTraceObject):
        self._rayTraceObjects.remove(obj)
        self._treesNeedRebuilding = True

    # RM:262-336 — flatten the registered objects into the lists the buffers are made from; normals (RM:340-368) and the
    # object-level BVHs (RM:405-722 output contract) come from the C++ host library (csrc/host_scene.cpp)
    def RebuildObjectLists(self, literal_leaf_bounds: bool = False, pairing_heap: bool = False):
        s = self.scene
        self._drop_normals_plans()                                                # the spans and the weld they were made for are gone
        spheres, mesh_objects, verts, idx = [], [], [], []
        nv = ni = 0
        for obj in self._rayTraceObjects:
            lighting = scenes._params(obj.albedoColor, obj.specularColor, obj.emissionColor, obj.smoothness)
            if obj.type == 1:                                                     # RM:277-293
                sp = np.zeros((), scenes.SPHERE_DT)
                sp["position"], sp["radius"], sp["lighting"] = obj.position, obj.radius, lighting
                spheres.append(sp)
            else:                                                                 # RM:295-321
                v = np.asarray(obj.vertices, np.float32).reshape(-1, 3)
                t = np.asarray(obj.triangles, np.int32).reshape(-1)
                mo = np.zeros((), scenes.MESHOBJECT_DT)
                mo["localToWorldMatrix"], mo["indices_offset"], mo["indices_count"], mo["lighting"] = obj.localToWorldMatrix, ni, len(t), lighting
                verts.append(v)
                idx.append(t + nv)                                                # RM:305: offset by the first vertex
                mesh_objects.append(mo)
                nv += len(v)
                ni += len(t)
        s.spheres = np.array(spheres, scenes.SPHERE_DT) if spheres else np.zeros(0, scenes.SPHERE_DT)
        s.mesh_objects = np.array(mesh_objects, scenes.MESHOBJECT_DT) if mesh_objects else np.zeros(0, scenes.MESHOBJECT_DT)
        s.vertices = np.concatenate(verts) if verts else np.zeros((0, 3), np.float32)
        s.indices = np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32)
        s.normals = host_scene.compute_normals(s.vertices, s.indices)            # RM:328
        # CreateBVH(_meshObjects) / CreateBVH(_spheres), RM:727-728 (the reference throws on an empty list, A.7; here empty = no buffer)
        s.mesh_bvh = host_scene.build_object_bvh(host_scene.mesh_leaf_bounds(s.mesh_objects, s.vertices, s.indices, literal_leaf_bounds), pairing_heap) \
            if len(s.mesh_objects) else np.zeros(0, scenes.BVHNODE_DT)
        s.sphere_bvh = host_scene.build_object_bvh(host_scene.sphere_leaf_bounds(s.spheres, literal_leaf_bounds), pairing_heap) \
            if len(s.spheres) else np.zeros(0, scenes.BVHNODE_DT)
        self._heapsBehind = [False, False]                                        # the lists are the newest heaps again
        self._geometryBehind = False                                              # ... and the newest geometry
        if getattr(self, "rayDebug", None) is not None:                             # RM:331-335
            self.rayDebug.LogSceneCounts(len(s.spheres), len(s.mesh_objects), len(s.vertices), len(s.indices), len(s.normals))

    # RM:233-252
    def CreateComputeBuffer(self, buffer, data: np.ndarray, stride: int):
        count = data.nbytes // stride
        if buffer is not None and (count == 0 or buffer.count != count or buffer.stride != stride):
            buffer.Release()
            buffer = None
        if count != 0:
            if buffer is None:
                buffer = ComputeBuffer(self.ctx, count, stride)
            buffer.SetData(data)
        return buffer

    # RM:255-259
    def SetComputeBuffer(self, name: str, buffer):
        if buffer is not None:
            self.RayTraceShader.SetBuffer(0, name, buffer)

    # RM:725-746 (upload half)
    @staticmethod
    def tree_depth(n_objects: int) -> int:
        """MeshDepth / SphereDepth of CreateBVH (RM:683,705): ceil(log2 n) + 1 levels; 0 for an empty list."""
        return 0 if n_objects <= 0 else int(math.ceil(math.log2(n_objects))) + 1 if n_objects > 1 else 1

    def RebuildTrees(self):
        s = self.scene
        if self.device_object_heaps:                                              # never upload a host heap that is behind the device's
            self.SyncObjectHeaps()
        self.SyncGeometry()                                                       # ... nor geometry that is
        if self.rayDebug is not None:                                             # RM:731-735
            self.rayDebug.LogTreeReport(len(s.mesh_objects), self.tree_depth(len(s.mesh_objects)), len(s.mesh_bvh),
                                        len(s.spheres), self.tree_depth(len(s.spheres)), len(s.sphere_bvh))
        self._meshObjectBuffer = self.CreateComputeBuffer(self._meshObjectBuffer, s.mesh_objects, self.MeshObjectStructSize)
        self._vertexBuffer = self.CreateComputeBuffer(self._vertexBuffer, np.ascontiguousarray(s.vertices, np.float32), 12)
        self._indexBuffer = self.CreateComputeBuffer(self._indexBuffer, np.ascontiguousarray(s.indices, np.int32), 4)
        self._normalBuffer = self.CreateComputeBuffer(self._normalBuffer, np.ascontiguousarray(s.normals, np.float32), 12)
        self._sphereBuffer = self.CreateComputeBuffer(self._sphereBuffer, s.spheres, self.SphereStructSize)
        self._meshObjectBVHBuffer = self.CreateComputeBuffer(self._meshObjectBVHBuffer, s.mesh_bvh, self.BVHNodeSize)
        self._sphereBVHBuffer = self.CreateComputeBuffer(self._sphereBVHBuffer, s.sphere_bvh, self.BVHNodeSize)
        if self.SkyboxTexture is None and s.sky is not None:
            h, w = s.sky.shape[:2]
            self.SkyboxTexture = RenderTexture(self.ctx, w, h)
            self.SkyboxTexture.SetPixels(s.sky)

    # RM:772-795
    def SetShaderParameters(self):
        sh, s = self.RayTraceShader, self.scene
        sh.SetMatrix("_CameraToWorld", s.camera_to_world)
        sh.SetMatrix("_CameraInverseProjection", s.camera_inverse_projection)
        sh.SetTexture(0, "_SkyboxTexture", self.SkyboxTexture)
        ox, oy, seed = scenes.frame_uniforms(self._frame, self.frame_seed) if self._frame else (s.pixel_offset[0], s.pixel_offset[1], s.seed)
        sh.SetVector("_PixelOffset", (ox, oy))
        sh.SetFloat("_Seed", seed)
        # RM re-sets the four ints and the seven bindings every frame; setting a name to the value it has is a no-op at the boundary, and
        # when none of them changed since the last frame of this master the eleven calls are skipped as one (host time per frame is GPU
        # idle time before a batch of deferred frames is submitted: 9.4 -> ~5 us)
        key = (self.numBounces, self.numRays, len(s.mesh_bvh), len(s.sphere_bvh), self._meshObjectBuffer, self._vertexBuffer, self._indexBuffer,
               self._normalBuffer, self._sphereBuffer, self._meshObjectBVHBuffer, self._sphereBVHBuffer, id(sh._bound))
        if key == self._bindings_key and sh._bound.get("owner") is self:
            return
        sh.SetInt("_numBounces", self.numBounces)
        sh.SetInt("_numRays", self.numRays)
        sh.SetInt("_MeshBVH_len", len(s.mesh_bvh))
        sh.SetInt("_SphereBVH_len", len(s.sphere_bvh))
        self.SetComputeBuffer("_MeshObjects", self._meshObjectBuffer)
        self.SetComputeBuffer("_Vertices", self._vertexBuffer)
        self.SetComputeBuffer("_Indices", self._indexBuffer)
        self.SetComputeBuffer("_Normals", self._normalBuffer)
        self.SetComputeBuffer("_Spheres", self._sphereBuffer)
        self.SetComputeBuffer("_MeshBVH", self._meshObjectBVHBuffer)
        self.SetComputeBuffer("_SphereBVH", self._sphereBVHBuffer)
        self._bindings_key = key
        sh._bound["owner"] = self                               # another master (or direct Set* calls through another wrapper) on this context ends the shortcut

    # RM:824-845
    def InitRenderTexture(self):
        if self._target is None or self._target.width != self.screen_width or self._target.height != self.screen_height:
            if self._target is not None:
                self._target.Release()
                self._converged.Release()
            self._target = RenderTexture(self.ctx, self.screen_width, self.screen_height)
            self._converged = RenderTexture(self.ctx, self.screen_width, self.screen_height)
            self._currentSample = 0

    # RM:798-821
    def Render(self, destination: RenderTexture | None = None):
        self.InitRenderTexture()
        if self._temporal is not None:
            self._ensure_temporal_textures()
            if self._currentSample == 0:                                      # the accumulation restarted (rebuild, resize, reset): so do the counts
                self._tcount.SetPixels(np.zeros((self.screen_height, self.screen_width, 4), np.float32))
        self.RayTraceShader.SetTexture(0, "Result", self._target)
        threadGroupsX = math.ceil(self.screen_width / 8.0)
        threadGroupsY = math.ceil(self.screen_height / 8.0)
        if self.world_size == 1:
            self.RayTraceShader.Dispatch(0, threadGroupsX, threadGroupsY, 1)
        else:
            self.RayTraceShader.DispatchRows(0, threadGroupsX, threadGroupsY, 1, self.rank, self.world_size)
        if self._temporal is not None:
            self.ctx.blit_add_history(self._target, self._converged, self._tcount, self._temporal["max_history"])
        else:
            if self._additionMaterial is None:
                self._additionMaterial = Material("Hidden/AdditionShader")
            self._additionMaterial.SetFloat("_Sample", self._currentSample)
            Graphics.Blit(self._target, self._converged, self._additionMaterial)
        if destination is not None:
            Graphics.Blit(self._converged, destination)
        self._currentSample += 1
        self._frame += 1
        if self._mbAge is not None:
            self._mbAge += 1

    # RM:848-866
    def OnRenderImage(self, destination: RenderTexture | None = None):
        if self._treesNeedRebuilding:                                             # (tested here too: a frame pays no call for it)
            self._scene_ready()
        self.SetShaderParameters()
        self.Render(destination)

    # RM:850-859: the scene buffers exist once this has run; a rebuild restarts the accumulation
    def _scene_ready(self):
        if self._treesNeedRebuilding:
            self._currentSample = 0
            self._treesNeedRebuilding = False
            if self._rayTraceObjects:
                self.RebuildObjectLists()
            self.RebuildTrees()

    # The "Raycast" every engine binding offers (and the "test ray" of the reference's RayTraceDebug.cs:119-129): one closest-hit query
    # against the scene this master renders (include/urt.h urt_ray_query).  None for a miss, else the urt_RayHit fields as a dict.
    def Raycast(self, origin, direction, max_distance: float = math.inf):
        self._bind_for_queries()
        o = np.asarray(origin, dtype=np.float32).reshape(1, 3)
        d = np.asarray(direction, dtype=np.float32).reshape(1, 3)
        h = self.ctx.ray_query(o, d, t_max=float(max_distance))[0]
        if h["kind"] == 0:
            return None
        return {k: (h[k].copy() if h[k].shape else h[k].item()) for k in h.dtype.names}

    def _bind_for_queries(self):
        self._scene_ready()
        self.SetShaderParameters()

    # Path-traced radiance arriving along rays of the host's own — light probes, irradiance volumes, lightmap texels — with the scene
    # this master renders (include/urt.h urt_radiance_query): `samples` paths per ray of up to numBounces bounces, starting from the
    # current _Seed.  The "pixel" of query i is (i mod 4096, i div 4096) as floats, so every query has its own random stream.
    # origins, directions: (n, 3) float32 (numpy, or torch tensors on the context's device); returns (n, 4).
    def SampleRadiance(self, origins, directions, samples: int):
        self._bind_for_queries()
        n = int(origins.shape[0])
        seed = self.RayTraceShader._bound[("f", "_Seed")]                         # the float32 SetShaderParameters has just bound
        if type(origins).__module__.startswith("torch"):
            import torch
            i = torch.arange(n, dtype=torch.int64, device=origins.device)
            pixels = torch.stack([(i % 4096).to(torch.float32), (i // 4096).to(torch.float32)], dim=1)
        else:
            i = np.arange(n, dtype=np.int64)
            pixels = np.stack([(i % 4096).astype(np.float32), (i // 4096).astype(np.float32)], axis=1)
        return self.ctx.radiance_query(origins, directions, pixels, seed, samples, self.numBounces)

    # Fresh samples for chosen pixels of the camera this master renders with — e.g. the ones a reprojection left without history:
    # exactly what the next frame writes to them (urt_radiance_query, pixels mode, with numRays and numBounces).  xy: (n, 2) int32.
    def ResamplePixels(self, xy):
        self._bind_for_queries()
        self.InitRenderTexture()
        self.RayTraceShader.SetTexture(0, "Result", self._target)
        return self.ctx.radiance_query_pixels(xy, self.numRays, self.numBounces)

    # After MoveCamera / MoveObjects with temporal accumulation: fresh samples for the pixels the reprojection left with a count below
    # `below` (1.0: no history at all), selected, traced and blended into _converged and its count texture on the GPU (include/urt.h
    # urt_resample_below) — each gets what a frame of numRays x numBounces would write to it, under a fresh _Seed, as one frame's worth
    # (weight 1).  The host decides when to call it; returns the number of pixels resampled.
    def ResampleDisocclusions(self, below: float = 1.0) -> int:
        from ._lib import UrtError
        if self._temporal is None:
            raise UrtError(1, "ResampleDisocclusions: temporal accumulation is off (EnableTemporalAccumulation)")
        if self._converged is None or not self._converged.handle or self._tcount is None or self._currentSample == 0:
            raise UrtError(2, "ResampleDisocclusions: no accumulated image yet (render a frame first)")
        self._bind_for_queries()
        self.InitRenderTexture()
        self.RayTraceShader.SetTexture(0, "Result", self._target)
        return self.ctx.resample_below(self._converged, self._tcount, below, self.numRays, self.numBounces, 1.0, self._temporal["max_history"])

    # Per-pixel first-hit feature buffers of the camera this master renders with (include/urt.h urt_render_aov): hit, normal, albedo and
    # id textures of the screen size, re-created with it as InitRenderTexture re-creates the frame's (RM:834-840).  A host calls it when
    # the camera moves — when the accumulation resets too.  Returns the four RenderTextures (filled once the deferred work has run:
    # GetPixels waits for it).
    def RenderFeatureBuffers(self, frame_ray: bool = False):
        self._bind_for_queries()
        self._aov = self._sized(self._aov, self.screen_width, self.screen_height, 4)
        self.ctx.render_aov(*self._aov, frame_ray=frame_ray)
        return self._aov

    # A texture this master owns (or, with n, a tuple of n of one size) at width x height: the one given if it has that size, else it
    # is released and a new one made — as InitRenderTexture re-creates the frame's with the screen (RM:834-840).
    def _sized(self, owned, width: int, height: int, n: int | None = None):
        held = () if owned is None else owned if n else (owned,)
        if held and (held[0].width, held[0].height) == (width, height):
            return owned
        for t in held:
            t.Release()
        made = tuple(RenderTexture(self.ctx, width, height) for _ in range(n or 1))
        return made if n else made[0]

    # The destination argument of Denoise, Upscale and ToneMap: None, or a live RenderTexture of this master's context (the callers
    # check its size)
    def _destination_arg(self, destination, who: str):
        if destination is not None and not isinstance(destination, RenderTexture):
            raise TypeError(f"{who}: destination must be a RenderTexture or None, not {type(destination).__name__}")
        if destination is not None and (destination.ctx is not self.ctx or not destination.handle):
            raise ValueError(f"{who}: destination belongs to another context or was released")

    # Feature buffers through the centres of the frames' samples (_sample_centre_projection below), for each (width, height, targets of
    # render_aov) in turn; the host's _CameraInverseProjection is bound again afterwards, whatever happens.
    def _render_through_sample_centres(self, *renders):
        try:
            for width, height, targets in renders:
                self.RayTraceShader.SetMatrix("_CameraInverseProjection", self._sample_centre_projection(width, height))
                self.ctx.render_aov(*targets)
        finally:
            self.RayTraceShader.SetMatrix("_CameraInverseProjection", self.scene.camera_inverse_projection)

    # The progressive image `_converged` (RM:12), denoised with this master's feature buffers as guides (include/urt.h urt_denoise):
    # hit, normal and albedo of RenderFeatureBuffers, rendered here when they do not exist yet or have another size (a host refreshes
    # them when the camera moves).  Writes into `destination`, or into a screen-sized texture this master owns, and returns it.
    # params: iterations, sigma_color, sigma_normal, sigma_depth of Context.denoise.
    def Denoise(self, destination: RenderTexture | None = None, **params):
        from ._lib import UrtError
        if self._converged is None or not self._converged.handle:
            raise UrtError(2, "Denoise: no accumulated image yet (render a frame first)")
        self._destination_arg(destination, "Denoise")
        denoise_params(**params)                                                  # checked before anything reaches the library
        if self._aov is None or self._aov[0].width != self._converged.width or self._aov[0].height != self._converged.height:
            self.RenderFeatureBuffers()
        if destination is None:
            destination = self._denoised = self._sized(self._denoised, self._converged.width, self._converged.height)
        hit, normal, albedo, _ = self._aov
        self.ctx.denoise(self._converged, destination, hit, normal, albedo, **params)
        return destination

    # Trace at low resolution, present at full (include/urt.h urt_upsample; no counterpart in the reference): the progressive image
    # `_converged`, traced at screen_width x screen_height, reconstructed at width x height with this master's feature buffers on both
    # grids as guides, rendered here into textures this master owns, through the centres of the frames' samples rather than the pixel
    # centres (_sample_centre_projection below; RenderFeatureBuffers' own textures are left as they are).  Opt-in:
    # Render is untouched and screen_width / screen_height stay the traced size.  Writes into `destination` (width x height), or into a
    # texture this master owns, and returns it; the per-pixel count goes to a count texture this master owns (_upcount): the low image's
    # counts with temporal accumulation on, else _currentSample scaled by the ratio of the pixel counts.  Sky pixels take the exact sky
    # from the full-size albedo buffer.  fill_holes: the pixels left with a count below `below` (1.0: the ones no low-resolution tap
    # could serve) get one frame's worth of full-resolution paths (urt_resample_below), a full-size texture of this master bound as
    # Result — Render rebinds its own on the next frame; their number is kept in upscaleFilled.  params: normal_threshold,
    # plane_threshold, wide_fallback of Context.upsample.  A host calls it per presented frame; both sets of guides are rendered anew
    # on every call, so a moved camera or scene needs nothing more.
    def Upscale(self, width: int, height: int, destination: RenderTexture | None = None, fill_holes: bool = False, below: float = 1.0, **params):
        from ._lib import UrtError
        from .unity_api import upsample_params, _number_arg
        if self._converged is None or not self._converged.handle or self._currentSample == 0:
            raise UrtError(2, "Upscale: no accumulated image yet (render a frame first)")
        for name, v in (("width", width), ("height", height)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"Upscale: {name} must be an int, not {type(v).__name__}")
            if v <= 0:
                raise ValueError(f"Upscale: {name} must be positive, not {v}")
        width, height = int(width), int(height)
        self._destination_arg(destination, "Upscale")
        if destination is not None and (destination.width, destination.height) != (width, height):
            raise ValueError(f"Upscale: destination is {destination.width} x {destination.height}, not {width} x {height}")
        if not isinstance(fill_holes, (bool, np.bool_)):
            raise TypeError(f"Upscale: fill_holes must be a bool, not {type(fill_holes).__name__}")
        below = _number_arg(below, "below", "Upscale")
        unknown = set(params) - {"normal_threshold", "plane_threshold", "wide_fallback"}
        if unknown:
            raise TypeError(f"Upscale: unknown parameters {sorted(unknown)}")
        upsample_params(**params)                                                 # checked before anything reaches the library
        self._bind_for_queries()
        if self._currentSample == 0:
            raise UrtError(2, "Upscale: the scene changed and no frame has been rendered since")
        if self._upaov is None or (self._upaov[0].width, self._upaov[0].height) != (width, height) \
                or (self._uplow[0].width, self._uplow[0].height) != (self.screen_width, self.screen_height):
            self._release_upscale()
            self._uplow = tuple(RenderTexture(self.ctx, self.screen_width, self.screen_height) for _ in range(4))
            self._upaov = tuple(RenderTexture(self.ctx, width, height) for _ in range(4))
            self._upcount = RenderTexture(self.ctx, width, height)
        low_hit, low_normal, _, low_id = self._uplow
        hit, normal, albedo, ids = self._upaov
        self._render_through_sample_centres((self.screen_width, self.screen_height, self._uplow), (width, height, self._upaov))
        if destination is None:
            if self._upscaled is None:
                self._upscaled = RenderTexture(self.ctx, width, height)
            destination = self._upscaled
        if self._temporal is not None and self._tcount is not None:
            counts = {"low_count": self._tcount}
        else:
            counts = {"count_scale": float(self._currentSample) * (self.screen_width * self.screen_height) / (width * height)}
        self.ctx.upsample(self._converged, low_hit, low_normal, low_id, hit, normal, ids, destination, self._upcount, albedo=albedo,
                          sky_from_albedo=True, **counts, **params)
        self.upscaleFilled = 0
        if fill_holes:
            if self._uptarget is None:
                self._uptarget = RenderTexture(self.ctx, width, height)
            self.RayTraceShader.SetTexture(0, "Result", self._uptarget)
            self.upscaleFilled = self.ctx.resample_below(destination, self._upcount, below, self.numRays, self.numBounces, 1.0, 0.0)
        return destination

    # A frame places the sample of pixel (x, y) at (x + rand + _PixelOffset.x, y + rand + _PixelOffset.y) with both terms in [0, 1)
    # (RS:448-449, csrc/camera_device.h jitter_uv): an accumulated image is a tent-filtered view centred on (x + 1, y + 1), half a pixel
    # OF ITS OWN GRID from the pixel centre (x + 0.5, y + 0.5) that urt_render_aov(URT_AOV_PIXEL_CENTER) looks through.  On a low grid
    # that half pixel is a whole pixel of the presented image, so guides through the pixel centres would label every low texel with the
    # surface one presented pixel beside the one it holds.  This is _CameraInverseProjection with the uv moved by half a pixel of a
    # width x height grid (u = s / width * 2 - 1: 1 / width), so that the pixel-centre ray of (x, y) goes through (x + 1, y + 1).
    def _sample_centre_projection(self, width: int, height: int) -> np.ndarray:
        p = np.array(self.scene.camera_inverse_projection, dtype=np.float32).reshape(16).copy()
        p[12:16] += p[0:4] * np.float32(1.0 / width) + p[4:8] * np.float32(1.0 / height)
        return p

    def _release_upscale(self):
        for t in (self._uplow or ()) + (self._upaov or ()) + (self._upcount, self._upscaled, self._uptarget):
            if t is not None:
                t.Release()
        self._uplow = self._upaov = self._upcount = self._upscaled = self._uptarget = None

    # ---- auto-exposure and tone mapping (include/urt.h urt_auto_exposure / urt_tonemap; no counterpart in the reference, whose
    # _converged goes to an HDR camera target) ----
    # Opt-in, for a host that presents 8 bits: ToneMap brings the progressive image `_converged` into [0, 1] — with auto-exposure on it
    # first meters it (with temporal accumulation on, only the pixels that hold samples) — and writes `destination`, or a texture of
    # _converged's size this master owns, and returns it; a formatted readback of that texture (RGBA8 sRGB) is the presented frame.
    # _converged itself is never modified, Render / OnRenderImage are untouched.  params: the fields of urt_ExposureParams; the state
    # starts fresh, so the first metering snaps to its target whatever `rate` is.
    def EnableAutoExposure(self, **params):
        import torch
        from .unity_api import exposure_params
        exposure_params(**params)                                                 # checked before anything is created
        self._exposure = dict(params)
        self._exposureState = torch.zeros(260, dtype=torch.int32, device=torch.device("cuda", self.ctx.device))   # a urt_ExposureState

    def DisableAutoExposure(self):
        self._exposure = self._exposureState = None

    # Bloom (include/urt.h urt_bloom), opt-in as well: with it on, ToneMap puts _converged + bloom into its destination (threshold and
    # clamp in the units of the metered exposure when auto-exposure is on) and tone-maps the destination in place; with it off ToneMap
    # enqueues what it always did.  params: the fields of urt_BloomParams.  Nothing is created here: the pyramid is the context's scratch.
    def EnableBloom(self, **params):
        from .unity_api import bloom_params
        bloom_params(**params)                                                    # checked at once
        self._bloom = dict(params)

    def DisableBloom(self):
        self._bloom = None

    # Depth of field (include/urt.h urt_depth_of_field), opt-in as well: with it on, ToneMap renders the hit guide of the bound camera
    # into a texture of _converged's size this master owns — through the centres of the frames' samples, as Upscale's guides
    # (_sample_centre_projection), the host's _CameraInverseProjection bound again afterwards — puts the blurred _converged into its
    # destination, and bloom (if enabled) and the tone mapping follow in place.  With it off ToneMap enqueues what it always did.
    # params: the fields of urt_DofParams; unity_api.dof_scale gives `scale` for a physical camera.  Focus and aperture change between
    # two ToneMap calls without a ray being traced: _converged is never modified.  Nothing is created here.
    def EnableDepthOfField(self, **params):
        from .unity_api import dof_params
        dof_params(**params)                                                      # checked at once
        self._dof = dict(params)

    def DisableDepthOfField(self):
        self._dof = None

    def _release_dof(self):
        if self._dofHit is not None:
            self._dofHit.Release()
        self._dofHit = None

    # Motion blur (include/urt.h urt_motion_blur), opt-in as well and only with temporal accumulation on, whose reprojection is where
    # the motion vectors come from: with it on, every edit that keeps history (MoveCamera, MoveObjects, DeformMeshes, SkinMeshes,
    # MorphMeshes) has its reprojection write the motion image into a texture this master owns, and ToneMap streaks the image along it
    # — after the depth of field, ahead of the bloom, with the hit guide the depth of field uses — while that motion is no older than
    # one rendered frame.  A still view therefore presents unblurred; a host that edits every frame gets a streak every frame.  With
    # it off the master issues the calls it always did.  params: the fields of urt_MotionBlurParams.  Nothing is created here.
    def EnableMotionBlur(self, **params):
        from .unity_api import motion_blur_params
        motion_blur_params(**params)                                              # checked at once
        if self._temporal is None:
            raise ValueError("EnableMotionBlur: temporal accumulation is off (EnableTemporalAccumulation first): without a reprojection "
                             "there are no motion vectors")
        self._mblur = dict(params)

    def DisableMotionBlur(self):
        self._mblur = None
        self._mbAge = None

    def _release_motion_blur(self):
        for t in (self._mbMotion, self._mbStage):
            if t is not None:
                t.Release()
        self._mbMotion = self._mbStage = self._mbAge = None

    def _motion_is_fresh(self) -> bool:
        return self._mblur is not None and self._mbAge is not None and self._mbAge <= 1 and self._mbMotion is not None \
            and (self._mbMotion.width, self._mbMotion.height) == (self._converged.width, self._converged.height)

    def ToneMap(self, destination: RenderTexture | None = None, operator="aces", exposure: float = 1.0, white: float = 4.0):
        from ._lib import UrtError
        from .unity_api import tonemap_params
        if self._converged is None or not self._converged.handle:
            raise UrtError(2, "ToneMap: no accumulated image yet (render a frame first)")
        self._destination_arg(destination, "ToneMap")
        if destination is self._converged:
            raise ValueError("ToneMap: destination is the accumulated image")
        if destination is not None and (destination.width, destination.height) != (self._converged.width, self._converged.height):
            raise ValueError(f"ToneMap: destination is {destination.width} x {destination.height}, not "
                             f"{self._converged.width} x {self._converged.height}")
        params = {"op": operator, "exposure": exposure, "white": white}
        tonemap_params(**params)                                                  # checked before anything reaches the library
        if destination is None:
            destination = self._tonemapped = self._sized(self._tonemapped, self._converged.width, self._converged.height)
        if self._exposure is not None:
            count = self._tcount if self._temporal is not None else None
            self.ctx.auto_exposure(self._converged, self._exposureState, count, **self._exposure)
        state = self._exposureState if self._exposure is not None else None
        source = self._converged
        streak = self._motion_is_fresh()
        if self._dof is not None or streak:
            width, height = self._converged.width, self._converged.height
            self._bind_for_queries()
            self._dofHit = self._sized(self._dofHit, width, height)
            self._render_through_sample_centres((width, height, (self._dofHit,)))
        if self._dof is not None:
            if streak:                                                            # the streak has no in-place form: it reads a stage of this master's
                self._mbStage = self._sized(self._mbStage, width, height)
            source = self._mbStage if streak else destination
            self.ctx.depth_of_field(self._converged, self._dofHit, source, **self._dof)
        if streak:
            self.ctx.motion_blur(source, self._mbMotion, self._dofHit, destination, **self._mblur)
            source = destination
        if self._bloom is not None:
            self.ctx.bloom(source, destination, state, **self._bloom)
            source = destination
        self.ctx.tonemap(source, destination, state, **params)
        return destination

    # RM:760-769: a camera move resets the running mean
    def ResetAccumulation(self):
        self._currentSample = 0

    # ---- temporal accumulation (no counterpart in the reference, which restarts the mean at every camera move, RM:765-767) ----
    # Opt-in: once enabled, every frame blends with a per-pixel sample count (include/urt.h urt_blit_add_history) and MoveCamera carries
    # the accumulated image into the new view (urt_reproject) instead of restarting it.  The settings are urt_ReprojectParams' (defaults:
    # include/urt.h URT_REPROJECT_DEFAULT_*); max_history also caps the count the blend uses, so a still view keeps a running mean of its
    # last max_history frames (0 = unlimited).
    def EnableTemporalAccumulation(self, max_history: float = None, normal_threshold: float = None, plane_threshold: float = None,
                                   moved_max_history: float = 0.0, deform_normal_threshold: float = None):
        from ._lib import REPROJECT_DEFAULTS
        mmh = _max_history_arg(moved_max_history, "EnableTemporalAccumulation", "moved_max_history")
        if deform_normal_threshold is not None:
            deform_normal_threshold = _number_arg(deform_normal_threshold, "deform_normal_threshold", "EnableTemporalAccumulation")
        given = {"max_history": max_history, "normal_threshold": normal_threshold, "plane_threshold": plane_threshold}
        settings = {k: (REPROJECT_DEFAULTS[k] if v is None else v) for k, v in given.items()}
        p = reproject_params(np.eye(4, dtype=np.float32).reshape(16), **settings)   # checked before anything is created
        self._temporal = {"max_history": p.max_history, "normal_threshold": p.normal_threshold, "plane_threshold": p.plane_threshold}
        self._moved_max_history = mmh
        self._deform_normal_threshold = deform_normal_threshold
        self._ensure_temporal_textures()
        self._tcount.SetPixels(np.zeros((self.screen_height, self.screen_width, 4), np.float32))   # creation is not assumed to zero
        self._currentSample = 0                                               # the count texture starts empty: so does the mean

    def DisableTemporalAccumulation(self):
        self._release_temporal()
        self._mblur = None                                                    # (no reprojection, no motion vectors)
        self._temporal = None
        self._currentSample = 0

    def _release_temporal(self):
        for t in (self._tcount,) + (self._tspare or ()) + sum(self._taov or (), ()):
            if t is not None:
                t.Release()
        self._tcount = self._tspare = self._taov = None
        self._release_motion_blur()
        for b in self._tmotion:
            if b is not None:
                b.Release()
        self._tmotion = [None, None]
        for b in self._tdeform:
            if b is not None:
                b.Release()
        self._tdeform = [None, None, None]

    # keep_history, before the edit: the vertex buffer as the history saw it is copied on the device into the previous-positions buffer
    # (include/urt.h urt_buffer_copy: no download) and the current _MeshObjects list becomes prev_mesh_objects.
    def _snapshot_for_deform(self):
        prev_v = self._tdeform[0]
        if prev_v is not None and prev_v.count != self._vertexBuffer.count:
            prev_v.Release()
            prev_v = None
        if prev_v is None:
            prev_v = ComputeBuffer(self.ctx, self._vertexBuffer.count, 12)
        self._tdeform[0] = prev_v
        prev_v.CopyFrom(self._vertexBuffer)
        self._tdeform[1] = self.CreateComputeBuffer(self._tdeform[1], self.scene.mesh_objects, 112)

    # keep_history, after the edit: the flags of the edited meshes; -> the deform argument of Context.reproject
    def _deform_argument(self, edited):
        flags = np.zeros(len(self.scene.mesh_objects), np.int32)
        flags[list(edited)] = 1
        self._tdeform[2] = self.CreateComputeBuffer(self._tdeform[2], flags, 4)
        d = (self._tdeform[0], self._indexBuffer, self._tdeform[1], self._tdeform[2])
        return d if self._deform_normal_threshold is None else d + (self._deform_normal_threshold,)

    def _ensure_temporal_textures(self):
        w, h = self.screen_width, self.screen_height
        if self._tcount is not None and (self._tcount.width, self._tcount.height) == (w, h):
            return
        self._release_temporal()
        self._tcount = RenderTexture(self.ctx, w, h)
        self._tspare = (RenderTexture(self.ctx, w, h), RenderTexture(self.ctx, w, h))
        self._taov = tuple(tuple(RenderTexture(self.ctx, w, h) for _ in range(3)) for _ in range(2))
        self._currentSample = 0                                               # a new count texture: the next frame zeroes it

    # ---- the protocol every edit that keeps history follows (MoveCamera, MoveObjects, DeformMeshes, SkinMeshes / MorphMeshes) ----
    # With _has_history(): _history_begin() renders the pixel-centre feature buffers of the scene and the camera as the history saw
    # them; the caller applies its edit (lists, uploads, the new camera matrices); _history_finish() renders the feature buffers of
    # what the next frame will see, uploads the motion tables of the edit, reprojects the accumulated image and its counts into the
    # spare pair and swaps the pairs, so that the next frame blends into the reprojected one.  Without history the caller applies its
    # edit and ends in ResetAccumulation().
    def _has_history(self) -> bool:
        return self._temporal is not None and self._converged is not None and self._currentSample > 0 and not self._treesNeedRebuilding \
            and (self._converged.width, self._converged.height) == (self.screen_width, self.screen_height)

    def _history_begin(self) -> np.ndarray:
        """-> the world-to-clip matrix of the camera the history was accumulated under, for _history_finish."""
        s = self.scene
        self._ensure_temporal_textures()
        prev_m = scenes.world_to_clip(s.camera_to_world, s.camera_inverse_projection)
        hit, normal, ids = self._taov[0]
        self.SetShaderParameters()
        self.ctx.render_aov(hit, normal, None, ids)
        return prev_m

    def _history_finish(self, prev_m, motion: dict | None = None):
        """motion: the keywords of _motion_arguments for an edit that moved or deformed objects.  None (a camera move) passes none of
        Context.reproject's motion keywords, which makes the call urt_reproject rather than urt_reproject_objects."""
        prev, cur = self._taov
        self.SetShaderParameters()
        self.ctx.render_aov(cur[0], cur[1], None, cur[2])
        moved = {} if motion is None else self._motion_arguments(**motion)
        color, count = self._tspare
        if self._mblur is not None:                                               # the motion image of this edit, for ToneMap's streak
            self._mbMotion = self._sized(self._mbMotion, self._converged.width, self._converged.height)
            moved["motion"] = self._mbMotion
            self._mbAge = 0
        self.ctx.reproject(self._converged, self._tcount, *prev, *cur, color, count, prev_m, **moved, **self._temporal)
        self._tspare = (self._converged, self._tcount)
        self._converged, self._tcount = color, count

    def _motion_arguments(self, mesh=None, sphere=None, deformed=(), keep: bool = False) -> dict:
        """Uploads the motion tables of an edit into _tmotion; -> the keywords of Context.reproject that name them.  mesh / sphere:
        MoveObjects' "current world -> previous world" tables, None for a kind nothing of which moved (a table of no rows makes
        CreateComputeBuffer release the buffer).  deformed: the meshes that changed shape and nothing else has moved — identity
        entries, all-NaN ("no history") for the deformed ones unless `keep`, which hands them to the per-vertex path instead."""
        s = self.scene
        if deformed:
            mesh = host_scene.mesh_motion(s.mesh_objects, s.mesh_objects)
            if not keep:
                mesh[list(deformed)] = np.nan
        for k, table in enumerate((mesh, sphere)):
            self._tmotion[k] = self.CreateComputeBuffer(self._tmotion[k], table if table is not None else np.zeros((0, 12), np.float32), 48)
        moved = {"mesh_motion": self._tmotion[0], "sphere_motion": self._tmotion[1], "moved_max_history": self._moved_max_history}
        if keep:
            moved["deform"] = self._deform_argument(deformed)
        return moved

    # A camera move.  camera_to_world / camera_inverse_projection: 16 floats each in Unity Matrix4x4 memory order (the inverse projection
    # stays when not given).  Temporal accumulation off: the new matrices and ResetAccumulation() (RM:765-767).  On: the pixel-centre
    # feature buffers of the previous and the new camera are rendered, the accumulated image and its counts are reprojected into the new
    # view, and the next frame blends into them.
    def MoveCamera(self, camera_to_world, camera_inverse_projection=None):
        s = self.scene
        c2w = np.ascontiguousarray(camera_to_world, dtype=np.float32).reshape(16).copy()
        invp = s.camera_inverse_projection if camera_inverse_projection is None else \
            np.ascontiguousarray(camera_inverse_projection, dtype=np.float32).reshape(16).copy()
        history = self._has_history()
        prev_m = self._history_begin() if history else None
        s.camera_to_world, s.camera_inverse_projection = c2w, invp
        if not history:
            self.ResetAccumulation()
            return
        self._history_finish(prev_m)

    # Objects move (and, optionally, the camera with them).  mesh_edits: {MeshObject index: 16-float localToWorldMatrix}; sphere_edits:
    # {sphere index: (position, radius)}.  The edits go into the scene's lists, the object-level heaps are rebuilt and everything is
    # re-uploaded through SetData as RebuildTrees does (moved meshes are refitted on the GPU, csrc/refit.hip).  Temporal accumulation
    # off, or no history yet: the accumulation restarts, the reference's behaviour for a moved object (RM:765-767).  On: the pixel-centre
    # feature buffers are rendered before the edits (old scene, old camera) and after them, the per-object "current world -> previous
    # world" tables are made from the two object lists (host_scene.mesh_motion / sphere_motion) and the accumulated image is reprojected
    # with them (include/urt.h urt_reproject_objects): a moved object keeps its history, clamped to moved_max_history when that is set.
    def MoveObjects(self, mesh_edits=None, sphere_edits=None, camera_to_world=None, camera_inverse_projection=None):
        s = self.scene
        mesh_edits = {} if mesh_edits is None else dict(mesh_edits)
        sphere_edits = {} if sphere_edits is None else dict(sphere_edits)
        if self._treesNeedRebuilding and self._rayTraceObjects:                    # the lists the indices refer to do not exist yet
            self.RebuildObjectLists()
        new_mo, new_sp = s.mesh_objects.copy(), s.spheres.copy()
        for what, edits, n in (("mesh_edits", mesh_edits, len(new_mo)), ("sphere_edits", sphere_edits, len(new_sp))):
            for k in edits:
                _index_arg(k, n, "MoveObjects", f"the keys of {what}", f"{what} names object")
        for k, mat in mesh_edits.items():
            new_mo[k]["localToWorldMatrix"] = _matrix16(mat, f"MoveObjects: mesh_edits[{k}]")
        for k, edit in sphere_edits.items():
            try:
                pos, radius = edit
                pos = np.asarray(pos, dtype=np.float32).reshape(3)
                radius = np.float32(radius)
            except (TypeError, ValueError):
                raise ValueError(f"MoveObjects: sphere_edits[{k}] must be (position of 3 floats, radius)") from None
            new_sp[k]["position"], new_sp[k]["radius"] = pos, radius
        c2w = s.camera_to_world if camera_to_world is None else _matrix16(camera_to_world, "MoveObjects: camera_to_world").copy()
        invp = s.camera_inverse_projection if camera_inverse_projection is None else \
            _matrix16(camera_inverse_projection, "MoveObjects: camera_inverse_projection").copy()
        history = self._has_history()
        prev_m = self._history_begin() if history else None
        prev_mo, prev_sp = s.mesh_objects, s.spheres
        self._apply_object_edits(new_mo, new_sp, mesh_edits, sphere_edits)
        s.camera_to_world, s.camera_inverse_projection = c2w, invp              # (before the second set of feature buffers)
        if not history:
            self.ResetAccumulation()
            return
        self._history_finish(prev_m, {"mesh": host_scene.mesh_motion(prev_mo, new_mo) if mesh_edits else None,
                                      "sphere": host_scene.sphere_motion(prev_sp, new_sp) if sphere_edits else None})

    def vertex_span(self, k: int) -> tuple:
        """(first, last) vertex the index range of MeshObject k refers to; (0, -1) when it has no triangle."""
        s = self.scene
        mo = s.mesh_objects[k]
        sl = np.asarray(s.indices[int(mo["indices_offset"]): int(mo["indices_offset"]) + int(mo["indices_count"]) // 3 * 3])
        return (int(sl.min()), int(sl.max())) if sl.size else (0, -1)

    # Meshes change SHAPE (skinning, cloth, blend shapes): edits = {MeshObject index: (n, 3) object-space positions for that mesh's vertex
    # span}, the span being the vertices its index range refers to, first to last (vertex_span).  The positions go into the scene's
    # vertex list and reach the library through ranged SetData, one call per span; with recompute_normals the normals are recomputed
    # (host_scene.compute_normals welds across meshes, so whatever changed is uploaded); the object-level heap is rebuilt from the new
    # bounds.  The library refits the deformed meshes on the GPU (include/urt.h option "refit_vertices").  Temporal accumulation off, or
    # no history yet: the accumulation restarts.  On: the MoveObjects protocol with an all-NaN motion entry for each deformed mesh, which
    # urt_reproject_objects defines as "no history": the deformed meshes restart at count 0, everything else keeps its history, and
    # ResampleDisocclusions fills them.  keep_history (needs temporal accumulation on, else it changes nothing): the deformed meshes keep
    # their history through per-vertex motion instead (include/urt.h urt_reproject_deformed) — the vertex buffer is snapshot on the
    # device before the edit, their motion entries are the identity and their pixels look up where their triangle's points were.
    def DeformMeshes(self, edits, recompute_normals: bool = True, keep_history: bool = False):
        s = self.scene
        edits = dict(edits)
        if self._treesNeedRebuilding and self._rayTraceObjects:                    # the lists the indices refer to do not exist yet
            self.RebuildObjectLists()
        n = len(s.mesh_objects)
        for k in edits:
            _index_arg(k, n, "DeformMeshes", "the keys of edits", "edits names MeshObject")
        spans, checked = {}, {}
        for k, pos in edits.items():
            lo, hi = spans[k] = self.vertex_span(k)
            try:
                a = np.ascontiguousarray(pos, dtype=np.float32)
            except (TypeError, ValueError):
                raise ValueError(f"DeformMeshes: edits[{k}] must be an (n, 3) array of positions") from None
            if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] != hi - lo + 1:
                raise ValueError(f"DeformMeshes: edits[{k}] must have shape ({hi - lo + 1}, 3), the vertex span of MeshObject {k}, not {a.shape}")
            checked[k] = a
        history = self._has_history()
        prev_m = self._history_begin() if history else None
        keep = bool(keep_history) and history and bool(edits) and self._vertexBuffer is not None and self._indexBuffer is not None
        if keep:
            self._snapshot_for_deform()
        vertices = np.array(s.vertices, dtype=np.float32).reshape(-1, 3)           # (a copy: the caller's scene arrays are not written)
        for k, a in checked.items():
            vertices[spans[k][0]: spans[k][1] + 1] = a
        s.vertices = vertices
        uploaded = not self._treesNeedRebuilding and self._vertexBuffer is not None      # else the next frame uploads everything anyway
        if uploaded:
            for k, a in checked.items():
                if len(a):
                    self._vertexBuffer.SetData(a, 0, spans[k][0], len(a))
        if recompute_normals:
            s.normals = host_scene.compute_normals(s.vertices, s.indices)
            if uploaded:
                self._normalBuffer = self.CreateComputeBuffer(self._normalBuffer, np.ascontiguousarray(s.normals, np.float32), 12)
        if edits:
            s.mesh_bvh = self._host_mesh_heap(s.mesh_objects)
            if self._rayTraceObjects:                                             # keep the registered objects in step with the lists
                meshes, first = [o for o in self._rayTraceObjects if o.type != 1], 0
                for o in meshes:
                    nv = len(np.asarray(o.vertices).reshape(-1, 3))
                    o.vertices = s.vertices[first: first + nv].copy()
                    first += nv
            if uploaded:
                self._meshObjectBVHBuffer = self.CreateComputeBuffer(self._meshObjectBVHBuffer, s.mesh_bvh, self.BVHNodeSize)
        if not history:
            self.ResetAccumulation()
            return
        self._history_finish(prev_m, {"deformed": edits, "keep": keep})

    # The meshes are REPLACED by geometry that lives in device memory (an LOD switch, procedurally generated or re-meshed geometry):
    # vertices / normals (stride 12) and indices (stride 4) are torch tensors on the context's device or (device address, element count)
    # pairs, mesh_objects the new MeshObject records (host data), mesh_bvh their object-level heap — or None with device_object_heaps,
    # which builds it where the buffers live.  A buffer whose count fits is reused; otherwise a new one is created, with SetDataDevice as
    # its first and only write, and the old one released.  The counts may all differ from the scene's: the next frame prepares from
    # scratch, and with device_prepare the geometry never crosses the bus.  The scene's vertices / indices / normals lists are BEHIND the
    # device afterwards (SyncGeometry() reads them back); skins, blend shapes and normals plans referred to the old vertex spans and
    # are dropped.  Topology changed, so no history is kept: the edit ends in ResetAccumulation(), as every edit without history does.
    def ReplaceGeometryDevice(self, vertices, indices, normals, mesh_objects, mesh_bvh=None):
        s = self.scene
        mo = np.ascontiguousarray(mesh_objects)
        if mo.dtype != scenes.MESHOBJECT_DT or mo.ndim != 1:
            raise ValueError("ReplaceGeometryDevice: mesh_objects must be a 1-d array of MeshObject records (scenes.MESHOBJECT_DT)")
        if mesh_bvh is None and not self.device_object_heaps:
            raise ValueError("ReplaceGeometryDevice: mesh_bvh is needed unless device_object_heaps is on (the host holds no positions to build it from)")
        if mesh_bvh is not None:
            mesh_bvh = np.ascontiguousarray(mesh_bvh)
            if mesh_bvh.dtype != scenes.BVHNODE_DT or mesh_bvh.ndim != 1:
                raise ValueError("ReplaceGeometryDevice: mesh_bvh must be a 1-d array of BVH nodes (scenes.BVHNODE_DT)")
        sources = [_device_list_arg(a, stride, name) for a, stride, name in ((vertices, 12, "vertices"), (indices, 4, "indices"), (normals, 12, "normals"))]
        if len(mo) and not all(count > 0 for _, count in sources):
            raise ValueError("ReplaceGeometryDevice: vertices, indices and normals must not be empty")
        if self._treesNeedRebuilding:                                             # the buffers of the other lists must exist, and no later rebuild may overwrite these
            self._scene_ready()
        old = [self._vertexBuffer, self._indexBuffer, self._normalBuffer]
        new = []
        for buf, (src, count), stride in zip(old, sources, (12, 4, 12)):
            if buf is None or buf.count != count:
                buf = ComputeBuffer(self.ctx, count, stride) if count else None
            if buf is not None:
                buf.SetDataDevice(src, 0, count)
            new.append(buf)
        self._vertexBuffer, self._indexBuffer, self._normalBuffer = new
        for a, b in zip(old, new):
            if a is not None and a is not b:
                a.Release()
        s.mesh_objects = mo.copy()
        self._meshObjectBuffer = self.CreateComputeBuffer(self._meshObjectBuffer, s.mesh_objects, self.MeshObjectStructSize)
        self._geometryBehind = True
        if mesh_bvh is not None:
            s.mesh_bvh = mesh_bvh.copy()
            self._meshObjectBVHBuffer = self.CreateComputeBuffer(self._meshObjectBVHBuffer, s.mesh_bvh, self.BVHNodeSize)
            self._heapsBehind[0] = False
        else:
            n = max(0, _lib.load().urt_host_object_bvh_length(len(mo)))
            s.mesh_bvh = np.zeros(n, scenes.BVHNODE_DT)                           # its length is what the shader is told; the contents are behind
            heap = self._meshObjectBVHBuffer
            if heap is not None and heap.count != n:
                heap.Release()
                heap = None
            if heap is None and n:
                heap = ComputeBuffer(self.ctx, n, self.BVHNodeSize)
            self._meshObjectBVHBuffer = heap
            if n:
                self._build_heap_on_device(0)
        # what referred to the old vertex spans
        self._skins, self._skinBoxes, self._boxCache = {}, {}, {}
        for b in tuple(self._skinBuffers or ()) + tuple(self._boneBuffers.values()):
            b.Release()
        self._skinBuffers, self._boneBuffers = None, {}
        self._drop_morphs()
        self._morphs = {}
        self._drop_normals_plans()
        self.ResetAccumulation()

    def SyncGeometry(self):
        """scene.vertices / indices / normals as the buffers hold them now, after ReplaceGeometryDevice left them behind the device
        (ComputeBuffer.GetData: synchronising downloads).  Nothing to do otherwise."""
        s = self.scene
        if not self._geometryBehind:
            return
        get = lambda b, dt, shape: (b.GetData().reshape(-1).view(dt) if b is not None else np.zeros(0, dt)).reshape(shape).copy()
        s.vertices = get(self._vertexBuffer, np.float32, (-1, 3))
        s.indices = get(self._indexBuffer, np.int32, (-1,))
        s.normals = get(self._normalBuffer, np.float32, (-1, 3))
        self._geometryBehind = False

    def _mesh_index_arg(self, k, who: str, what: str):
        _index_arg(k, len(self.scene.mesh_objects), who, what, f"{what} names MeshObject")

    # A mesh gets a skin: bone_indices (n, 4) int32 and bone_weights (n, 4) float32 for the n vertices of its vertex span (vertex_span).
    # The span's positions and normals as the scene holds them NOW are kept as the rest pose.  Nothing reaches the library before
    # SkinMeshes.  (The term rule — which of the four are live — is urt_skin_vertices', include/urt.h.)
    def AttachSkin(self, mesh_index: int, bone_indices, bone_weights):
        s = self.scene
        if self._treesNeedRebuilding and self._rayTraceObjects:                    # the lists the index refers to do not exist yet
            self.RebuildObjectLists()
        self._mesh_index_arg(mesh_index, "AttachSkin", "mesh_index")
        lo, hi = self.vertex_span(mesh_index)
        n = hi - lo + 1
        try:
            idx = np.ascontiguousarray(bone_indices, dtype=np.int32)
            wgt = np.ascontiguousarray(bone_weights, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError("AttachSkin: bone_indices / bone_weights must be (n, 4) arrays") from None
        for name, a in (("bone_indices", idx), ("bone_weights", wgt)):
            if a.ndim != 2 or a.shape != (n, 4):
                raise ValueError(f"AttachSkin: {name} must have shape ({n}, 4), the vertex span of MeshObject {mesh_index}, not {a.shape}")
        self._skins[int(mesh_index)] = {
            "span": (lo, hi), "indices": idx.copy(), "weights": wgt.copy(), "uploaded": False,
            "rest_vertices": np.array(np.asarray(s.vertices, np.float32).reshape(-1, 3)[lo: hi + 1]),
            "rest_normals": np.array(np.asarray(s.normals, np.float32).reshape(-1, 3)[lo: hi + 1])}

    def _ensure_skin_buffers(self):
        nv = self._vertexBuffer.count
        if self._skinBuffers is not None and self._skinBuffers[0].count != nv:
            for b in self._skinBuffers:
                b.Release()
            self._skinBuffers = None
        if self._skinBuffers is None:
            self._skinBuffers = tuple(ComputeBuffer(self.ctx, nv, stride) for stride in (12, 12, 16, 16))
            for sk in self._skins.values():
                sk["uploaded"] = False
        for sk in self._skins.values():
            if not sk["uploaded"] and sk["span"][1] >= sk["span"][0]:
                for b, key in zip(self._skinBuffers, ("rest_vertices", "rest_normals", "indices", "weights")):
                    b.SetData(sk[key], 0, sk["span"][0], len(sk[key]))
                sk["uploaded"] = True

    def _world_box(self, k: int, lo3, hi3):
        """The float32 box of the eight corners of an object-space box through MeshObject k's localToWorldMatrix: float64, rounded outward."""
        m = np.asarray(self.scene.mesh_objects[k]["localToWorldMatrix"], dtype=np.float64).reshape(4, 4).T
        c = np.array([[x, y, z] for x in (lo3[0], hi3[0]) for y in (lo3[1], hi3[1]) for z in (lo3[2], hi3[2])], dtype=np.float64)
        w = c @ m[:3, :3].T + m[:3, 3]
        return np.nextafter(w.min(axis=0).astype(np.float32), np.float32(-np.inf)), np.nextafter(w.max(axis=0).astype(np.float32), np.float32(np.inf))

    def _object_heap_with_skins(self):
        """The object-level heap of the meshes: the skinned ones from the bounds the GPU found, the others from the scene's lists (kept
        while their matrix and the vertex list stay the same)."""
        s = self.scene
        n = len(s.mesh_objects)
        lo, hi = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        for k in range(n):
            if k in self._skinBoxes:
                if self._skinBoxes[k] is not None:                                  # (None: no finite vertex — an empty box)
                    lo[k], hi[k] = self._world_box(k, *self._skinBoxes[k])
                continue
            key = (np.asarray(s.mesh_objects[k]["localToWorldMatrix"]).tobytes(), id(s.vertices))
            hit = self._boxCache.get(k)
            if hit is None or hit[0] != key:
                if self._rayTraceObjects:
                    leaf = host_scene.mesh_leaf_bounds(s.mesh_objects[k: k + 1], s.vertices, s.indices)
                    hit = (key, np.array(leaf["vmin"][0], np.float32), np.array(leaf["vmax"][0], np.float32))
                else:
                    l1, h1 = scenes.mesh_bounds(s.mesh_objects[k: k + 1], s.vertices, s.indices)
                    hit = (key, l1[0], h1[0])
                self._boxCache[k] = hit
            lo[k], hi[k] = hit[1], hit[2]
        if not self._rayTraceObjects:
            return scenes.build_object_bvh(lo, hi)
        leaves = np.zeros(n, dtype=scenes.BVHNODE_DT)
        leaves["vmin"], leaves["vmax"], leaves["index"] = lo, hi, np.arange(n)
        return host_scene.build_object_bvh(leaves)

    def _drop_normals_plans(self):
        for hit in self._normalsPlans.values():
            hit[1].Release()
        self._normalsPlans = {}

    # RayTraceMaster.ComputeNormals (RM:340-368) on the GPU, for meshes whose positions were written on the device (SkinMeshes, a
    # ComputeBuffer.SetDataDevice of the vertex buffer): the normals of the vertex spans of the named MeshObjects (default: all) are
    # recomputed from the vertex buffer's device side into the normal buffer's (include/urt.h urt_compute_normals), and the library
    # re-gathers the shading normals of the meshes they meet in place.  One plan per span, cached: made from the buffers as they are at
    # its first use (a synchronising set-up call; it welds against every mesh's index slots); all plans are dropped when the object lists
    # are rebuilt, and one whose buffers were replaced or whose scene holds another index list since is made anew.  A deformation that merges or splits coincident vertices needs new plans: _drop_normals_plans.
    # ComputeNormals welds across meshes: a mesh that holds a vertex at the position of a deformed mesh's vertex takes that mesh's faces,
    # so it is named too.  History is not touched — that is the caller's business, as with ComputeBuffer.SetDataDevice.
    def RecomputeNormals(self, mesh_indices=None):
        if self._treesNeedRebuilding and self._rayTraceObjects:
            self.RebuildObjectLists()
        ks = list(range(len(self.scene.mesh_objects))) if mesh_indices is None else list(mesh_indices)
        for k in ks:
            self._mesh_index_arg(k, "RecomputeNormals", "mesh_indices")
        if self._treesNeedRebuilding:                                             # the buffers the plans read must exist
            self._bind_for_queries()
        for k in ks:
            lo, hi = self.vertex_span(k)
            if hi < lo:
                continue
            key = (self._vertexBuffer.handle, self._indexBuffer.handle, lo, hi)
            hit = self._normalsPlans.get(int(k))
            if hit is None or hit[0] != key or hit[2] is not self.scene.indices:
                if hit is not None:
                    hit[1].Release()
                hit = (key, self.ctx.normals_plan(self._vertexBuffer, self._indexBuffer, lo, hi - lo + 1), self.scene.indices)
                self._normalsPlans[int(k)] = hit
            hit[1].compute(self._normalBuffer)

    # Skinned meshes move: poses = {MeshObject index: (n_bones, 12) bone matrices} for meshes that have a skin (AttachSkin); a bone is
    # urt_ObjectMotion's a[12] — three columns of the linear part, then the translation — from the mesh's object space to itself.
    # The DeformMeshes protocol without a host copy of the positions: the bones are uploaded (a few KB), every span is skinned on the GPU
    # into the device side of the vertex and the normal buffer (include/urt.h urt_skin_vertices), its bounds come back from the GPU
    # (urt_buffer_bounds), the object-level heap is rebuilt from the world box of their eight corners and uploaded, and the library refits
    # the skinned meshes in place without the positions ever crossing the bus.  The scene's vertex and normal lists keep what they held.
    # History is treated exactly as DeformMeshes treats it: all-NaN motion entries with temporal accumulation on, ResetAccumulation else.
    # recompute_normals: the bones carry rest normals through their linear part, which is right for rigid bones only; with True the
    # normals of the skinned spans come from RecomputeNormals of the skinned positions instead, as the reference computes its normals.
    # keep_history: as DeformMeshes' — the snapshot of the vertex buffer is a device-to-device copy, so the positions still never cross
    # the bus.
    def SkinMeshes(self, poses, recompute_normals: bool = False, keep_history: bool = False):
        poses = dict(poses)
        if self._treesNeedRebuilding and self._rayTraceObjects:
            self.RebuildObjectLists()
        checked = self._checked_poses(poses, "SkinMeshes")

        def skin():
            self._ensure_skin_buffers()
            rest_v, rest_n, idx, wgt = self._skinBuffers
            for k, a in checked.items():
                lo, hi = self._skins[k]["span"]
                if hi < lo:
                    continue
                self._boneBuffers[k] = self.CreateComputeBuffer(self._boneBuffers.get(k), a, 48)
                self.ctx.skin_vertices(rest_v, rest_n, idx, wgt, self._boneBuffers[k], lo, hi - lo + 1, self._vertexBuffer,
                                       None if recompute_normals else self._normalBuffer)
        self._deform_on_device({k: self._skins[k]["span"] for k in checked}, skin, recompute_normals, keep_history)

    def _checked_poses(self, poses, who: str):
        """poses = {MeshObject index: (n_bones, 12)} of meshes that have a skin -> {int: float32 array}, or the error SkinMeshes raises."""
        checked = {}
        for k, bones in poses.items():
            self._mesh_index_arg(k, who, "the keys of poses")
            if int(k) not in self._skins:
                raise ValueError(f"{who}: MeshObject {k} has no skin (AttachSkin)")
            try:
                a = np.ascontiguousarray(bones, dtype=np.float32)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: poses[{k}] must be an (n_bones, 12) array") from None
            if a.ndim != 2 or a.shape[1] != 12 or a.shape[0] < 1:
                raise ValueError(f"{who}: poses[{k}] must have shape (n_bones, 12) with n_bones >= 1, not {a.shape}")
            checked[int(k)] = a
        return checked

    # The protocol SkinMeshes and MorphMeshes share, for meshes whose vertex spans (spans = {MeshObject index: (lo, hi)}) a device-side
    # deformation rewrites: the previous feature buffers, the optional snapshot, deform() — which enqueues the deformation into the
    # device side of the vertex (and normal) buffer —, the optional RecomputeNormals, the spans' bounds from the GPU, the object-level
    # heap, the new feature buffers and the reprojection.  The arguments were checked by the caller.
    def _deform_on_device(self, spans, deform, recompute_normals: bool, keep_history: bool):
        s = self.scene
        if self._treesNeedRebuilding:                                             # the buffers the deformation writes into must exist
            self._bind_for_queries()
        # (the trees never need rebuilding here: _bind_for_queries has just cleared the flag — and zeroed _currentSample, so a rebuild
        # means no history, as in the other edits)
        history = self._has_history()
        prev_m = self._history_begin() if history else None
        keep = bool(keep_history) and history and bool(spans)
        if keep:
            self._snapshot_for_deform()
        deform()
        if recompute_normals:
            self.RecomputeNormals(list(spans))
        if spans and self._can_build_heaps_on_device(0):
            self._build_heap_on_device(0)
            spans_to_bound = {}
        else:
            spans_to_bound = spans
        for k, (lo, hi) in spans_to_bound.items():
            if hi < lo:
                continue
            lo3, hi3, n = self.ctx.buffer_bounds(self._vertexBuffer, lo, hi - lo + 1)
            self._skinBoxes[k] = (lo3, hi3) if n > 0 else None
        if spans_to_bound:
            s.mesh_bvh = self._object_heap_with_skins()
            self._meshObjectBVHBuffer = self.CreateComputeBuffer(self._meshObjectBVHBuffer, s.mesh_bvh, self.BVHNodeSize)
            self._heapsBehind[0] = False
        if not history:
            self.ResetAccumulation()
            return
        self._history_finish(prev_m, {"deformed": spans, "keep": keep})

    # A mesh gets blend shapes (morph targets): targets = [(delta_vertices (n, 3), delta_normals (n, 3) or None), ...], dense over the
    # n vertices of its vertex span as Mesh.GetBlendShapeFrameVertices returns them.  Rows whose six deltas all compare == 0 are dropped,
    # the rest become urt_MorphDeltas with absolute vertex numbers.  The span's positions and normals as the scene holds them NOW are
    # kept as the rest pose, as AttachSkin records it.  Nothing reaches the library before MorphMeshes.
    def AttachBlendShapes(self, mesh_index: int, targets):
        s = self.scene
        if self._treesNeedRebuilding and self._rayTraceObjects:                    # the lists the index refers to do not exist yet
            self.RebuildObjectLists()
        self._mesh_index_arg(mesh_index, "AttachBlendShapes", "mesh_index")
        lo, hi = self.vertex_span(mesh_index)
        n = hi - lo + 1
        if isinstance(targets, (str, bytes)) or not hasattr(targets, "__len__"):
            raise ValueError("AttachBlendShapes: targets must be a list of (delta_vertices, delta_normals or None)")
        if not 1 <= len(targets) <= _lib.MORPH_MAX_TARGETS:
            raise ValueError(f"AttachBlendShapes: 1 .. {_lib.MORPH_MAX_TARGETS} targets, not {len(targets)}")
        parts = []
        for t, pair in enumerate(targets):
            if isinstance(pair, (str, bytes, np.ndarray)) or not hasattr(pair, "__len__") or len(pair) != 2:
                raise ValueError(f"AttachBlendShapes: targets[{t}] must be a pair (delta_vertices, delta_normals or None)")
            try:
                dp = np.ascontiguousarray(pair[0], dtype=np.float32)
                dn = np.zeros((n, 3), np.float32) if pair[1] is None else np.ascontiguousarray(pair[1], dtype=np.float32)
            except (TypeError, ValueError):
                raise ValueError(f"AttachBlendShapes: the deltas of targets[{t}] must be (n, 3) arrays") from None
            for name, a in (("delta_vertices", dp), ("delta_normals", dn)):
                if a.ndim != 2 or a.shape != (n, 3):
                    raise ValueError(f"AttachBlendShapes: {name} of targets[{t}] must have shape ({n}, 3), the vertex span of MeshObject "
                                     f"{mesh_index}, not {a.shape}")
            rows = np.flatnonzero(~((dp == 0).all(axis=1) & (dn == 0).all(axis=1)))
            d = np.zeros(len(rows), dtype=np.dtype(_lib.MORPH_DELTA_DT))
            d["vertex"], d["target"], d["dp"], d["dn"] = lo + rows, t, dp[rows], dn[rows]
            parts.append(d)
        old = self._morphs.get(int(mesh_index))
        if old is not None and old["plan"] is not None:
            old["plan"].Release()
        self._morphs[int(mesh_index)] = {
            "span": (lo, hi), "deltas": np.concatenate(parts), "n_targets": len(targets), "plan": None, "uploaded": False,
            "rest_vertices": np.array(np.asarray(s.vertices, np.float32).reshape(-1, 3)[lo: hi + 1]),
            "rest_normals": np.array(np.asarray(s.normals, np.float32).reshape(-1, 3)[lo: hi + 1])}

    def _ensure_morph_buffers(self):
        nv = self._vertexBuffer.count
        if self._morphBuffers is not None and self._morphBuffers[0].count != nv:
            for b in self._morphBuffers:
                b.Release()
            self._morphBuffers = None
        if self._morphBuffers is None:
            self._morphBuffers = tuple(ComputeBuffer(self.ctx, nv, 12) for _ in range(4))
            for mp in self._morphs.values():
                mp["uploaded"] = False
        for mp in self._morphs.values():
            lo, hi = mp["span"]
            if mp["plan"] is None:
                mp["plan"] = self.ctx.morph_plan(mp["deltas"], mp["n_targets"], lo, hi - lo + 1)
            if not mp["uploaded"] and hi >= lo:
                for b, key in zip(self._morphBuffers, ("rest_vertices", "rest_normals")):
                    b.SetData(mp[key], 0, lo, len(mp[key]))
                mp["uploaded"] = True

    def _drop_morphs(self):
        for mp in self._morphs.values():
            if mp["plan"] is not None:
                mp["plan"].Release()
                mp["plan"] = None
        for b in tuple(self._morphBuffers or ()) + tuple(self._morphWeightBuffers.values()):
            if b is not None:
                b.Release()
        self._morphBuffers, self._morphWeightBuffers = None, {}

    # Blend shapes move: weights = {MeshObject index: (n_targets,) float32} for meshes that have blend shapes (AttachBlendShapes).  The
    # SkinMeshes protocol with urt_morph_vertices as the deformation: the weights are uploaded (a few bytes per target) and every span is
    # morphed on the GPU.  A mesh that is not named in `poses` is morphed straight into the device side of the vertex and the normal
    # buffer, its normals normalised (URT_MORPH_NORMALIZE).  A mesh that also has a skin (AttachSkin) and an entry in poses = {MeshObject
    # index: (n_bones, 12)} — every key of poses is a key of weights — is morphed, normals as they come, into a pair of intermediate
    # buffers that urt_skin_vertices then takes as its rest pose: blend shapes come before the bones, and since the skin reads device
    # mirrors the morphed rest pose never crosses the bus.  recompute_normals and keep_history: as SkinMeshes'.
    def MorphMeshes(self, weights, poses=None, recompute_normals: bool = False, keep_history: bool = False):
        weights, poses = dict(weights), dict(poses or {})
        if self._treesNeedRebuilding and self._rayTraceObjects:
            self.RebuildObjectLists()
        checked = {}
        for k, w in weights.items():
            self._mesh_index_arg(k, "MorphMeshes", "the keys of weights")
            if int(k) not in self._morphs:
                raise ValueError(f"MorphMeshes: MeshObject {k} has no blend shapes (AttachBlendShapes)")
            try:
                a = np.ascontiguousarray(w, dtype=np.float32)
            except (TypeError, ValueError):
                raise ValueError(f"MorphMeshes: weights[{k}] must be an (n_targets,) array") from None
            if a.shape != (self._morphs[int(k)]["n_targets"],):
                raise ValueError(f"MorphMeshes: weights[{k}] must have shape ({self._morphs[int(k)]['n_targets']},), one weight per target, not {a.shape}")
            checked[int(k)] = a
        bones = self._checked_poses(poses, "MorphMeshes")
        for k in bones:
            if k not in checked:
                raise ValueError(f"MorphMeshes: poses names MeshObject {k}, which weights does not")
            if self._skins[k]["span"] != self._morphs[k]["span"]:
                raise ValueError(f"MorphMeshes: the skin and the blend shapes of MeshObject {k} were attached to different vertex spans")

        def morph():
            self._ensure_morph_buffers()
            rest_v, rest_n, mid_v, mid_n = self._morphBuffers
            if bones:
                self._ensure_skin_buffers()
            for k, a in checked.items():
                lo, hi = self._morphs[k]["span"]
                if hi < lo:
                    continue
                self._morphWeightBuffers[k] = self.CreateComputeBuffer(self._morphWeightBuffers.get(k), a, 4)
                plan, wb = self._morphs[k]["plan"], self._morphWeightBuffers[k]
                if k not in bones:
                    if recompute_normals:
                        plan.morph(rest_v, None, wb, self._vertexBuffer, None)
                    else:
                        plan.morph(rest_v, rest_n, wb, self._vertexBuffer, self._normalBuffer, normalize=True)
                    continue
                if recompute_normals:
                    plan.morph(rest_v, None, wb, mid_v, None)
                else:
                    plan.morph(rest_v, rest_n, wb, mid_v, mid_n)
                self._boneBuffers[k] = self.CreateComputeBuffer(self._boneBuffers.get(k), bones[k], 48)
                self.ctx.skin_vertices(mid_v, None if recompute_normals else mid_n, self._skinBuffers[2], self._skinBuffers[3], self._boneBuffers[k],
                                       lo, hi - lo + 1, self._vertexBuffer, None if recompute_normals else self._normalBuffer)
        self._deform_on_device({k: self._morphs[k]["span"] for k in checked}, morph, recompute_normals, keep_history)

    # The object-level heap of a mesh / sphere list on the host: through the C++ host library for registered objects, as
    # RebuildObjectLists builds them, else with the builders of scenes.py that made the pre-flattened scene's.
    def _host_mesh_heap(self, mesh_objects) -> np.ndarray:
        s = self.scene
        if self._rayTraceObjects:
            return host_scene.build_object_bvh(host_scene.mesh_leaf_bounds(mesh_objects, s.vertices, s.indices))
        return scenes.build_object_bvh(*scenes.mesh_bounds(mesh_objects, s.vertices, s.indices))

    def _host_sphere_heap(self, spheres) -> np.ndarray:
        if self._rayTraceObjects:
            return host_scene.build_object_bvh(host_scene.sphere_leaf_bounds(spheres))
        return scenes.build_object_bvh(*scenes.sphere_bounds(spheres))

    # the edited lists become the scene's, with the object-level heaps RebuildObjectLists / the scene builders make for them, and are
    # uploaded (RebuildTrees: SetData of data a buffer already holds changes nothing)
    def _apply_object_edits(self, new_mo, new_sp, mesh_edits, sphere_edits):
        s = self.scene
        s.mesh_objects, s.spheres = new_mo, new_sp
        if self._rayTraceObjects:                                                 # keep the registered objects in step with the lists
            meshes = [o for o in self._rayTraceObjects if o.type != 1]
            spheres = [o for o in self._rayTraceObjects if o.type == 1]
            for k in mesh_edits:
                meshes[k].localToWorldMatrix = np.array(new_mo[k]["localToWorldMatrix"], np.float32)
            for k in sphere_edits:
                spheres[k].position, spheres[k].radius = tuple(float(v) for v in new_sp[k]["position"]), float(new_sp[k]["radius"])
        on_device = [bool(e) and not self._treesNeedRebuilding and self._can_build_heaps_on_device(k)
                     for k, e in enumerate((mesh_edits, sphere_edits))]
        on_host = [bool(e) and not d for e, d in zip((mesh_edits, sphere_edits), on_device)]
        if on_host[0]:
            s.mesh_bvh = self._host_mesh_heap(new_mo)
        if on_host[1]:
            s.sphere_bvh = self._host_sphere_heap(new_sp)
        self._heapsBehind = [b and not h for b, h in zip(self._heapsBehind, on_host)]   # the recomputed lists are the newest
        if not any(on_device):
            if not self._treesNeedRebuilding:                                      # else the next frame uploads everything anyway
                self.RebuildTrees()
            return
        # the edited lists go up by SetData as always; the heaps of the edited kinds are built where the buffers live.  (RebuildTrees
        # would read the heaps back first.)  An edited kind whose heap the device cannot build takes the host path, as without the flag.
        if on_host[0]:
            self._meshObjectBVHBuffer = self.CreateComputeBuffer(self._meshObjectBVHBuffer, s.mesh_bvh, self.BVHNodeSize)
        if on_host[1]:
            self._sphereBVHBuffer = self.CreateComputeBuffer(self._sphereBVHBuffer, s.sphere_bvh, self.BVHNodeSize)
        self._meshObjectBuffer = self.CreateComputeBuffer(self._meshObjectBuffer, s.mesh_objects, self.MeshObjectStructSize)
        self._sphereBuffer = self.CreateComputeBuffer(self._sphereBuffer, s.spheres, self.SphereStructSize)
        for k in (0, 1):
            if on_device[k]:
                self._build_heap_on_device(k)

    # ---- device_object_heaps: the object-level heaps built where the buffers live (kind 0 = meshes, 1 = spheres) ----
    def _can_build_heaps_on_device(self, kind: int) -> bool:
        """The flag is set and the buffers the device builder reads and writes exist (RebuildTrees has made them)."""
        if not self.device_object_heaps:
            return False
        if kind == 0:
            need = (self._meshObjectBuffer, self._vertexBuffer, self._indexBuffer, self._meshObjectBVHBuffer)
        else:
            need = (self._sphereBuffer, self._sphereBVHBuffer)
        return all(b is not None for b in need)

    def _build_heap_on_device(self, kind: int):
        """Leaf boxes, then the heap into the bound heap buffer's device side: three (spheres: two) kernels on the context's stream, nothing
        waited for.  The library takes the heap at the next preparation, through the download every device-written small table gets."""
        objects, heap = (self._meshObjectBuffer, self._meshObjectBVHBuffer) if kind == 0 else (self._sphereBuffer, self._sphereBVHBuffer)
        leaves = self._leafBuffers[kind]
        if leaves is not None and leaves.count != objects.count:
            leaves.Release()
            leaves = None
        if leaves is None:
            leaves = self._leafBuffers[kind] = ComputeBuffer(self.ctx, objects.count, self.BVHNodeSize)
        if kind == 0:
            self.ctx.mesh_leaf_bounds(objects, self._vertexBuffer, self._indexBuffer, leaves)
        else:
            self.ctx.sphere_leaf_bounds(objects, leaves)
        self.ctx.build_object_bvh(leaves, heap)
        self._heapsBehind[kind] = True

    def SyncObjectHeaps(self, meshes: bool = True, spheres: bool = True):
        """scene.mesh_bvh / scene.sphere_bvh as the heap buffers hold them now: reads back the heaps that device_object_heaps built on the
        GPU (ComputeBuffer.GetData: a synchronising download).  Nothing to do for a heap the host built."""
        s = self.scene
        if meshes and self._heapsBehind[0] and self._meshObjectBVHBuffer is not None:
            s.mesh_bvh = self._meshObjectBVHBuffer.GetData().reshape(-1).view(scenes.BVHNODE_DT).copy()
            self._heapsBehind[0] = False
        if spheres and self._heapsBehind[1] and self._sphereBVHBuffer is not None:
            s.sphere_bvh = self._sphereBVHBuffer.GetData().reshape(-1).view(scenes.BVHNODE_DT).copy()
            self._heapsBehind[1] = False

    # RM:761-763: F12 -> ScreenCapture.CaptureScreenshot("Screenshots/" + Time.time + "-" + _currentSample + ".png")
    def CaptureScreenshot(self, directory: str, time_seconds: float) -> str:
        import os
        from . import host_io
        os.makedirs(directory, exist_ok=True)
        path = os.path.join(directory, f"{time_seconds:g}-{self._currentSample}.png")
        host_io.write_png(path, self._converged.GetPixels())
        return path

    # RM:869-878: the editor gizmos become text dumps of the two object-level heaps (RayTraceDebug.DrawBVHTree) and of the normals (DrawNormals)
    def OnDrawGizmos(self):
        if self.rayDebug is not None:
            s = self.scene
            self.rayDebug.DrawBVHTree(s.mesh_bvh, self.tree_depth(len(s.mesh_objects)), 0)
            mesh_dump = getattr(self.rayDebug, "last_dump", None)
            self.rayDebug.DrawBVHTree(s.sphere_bvh, self.tree_depth(len(s.spheres)), 1)
            if len(s.mesh_objects):
                self.rayDebug.DrawNormals(s.mesh_objects, s.vertices, s.indices, s.normals)      # RM:875-876
            return mesh_dump, getattr(self.rayDebug, "last_dump", None)
        return None, None

    # ---- checkpoint / resume of a progressive accumulation (the reference keeps `_converged` only in GPU memory and loses it
    # on every reset, RM:189,766,843,852; a 1024-spp run such as BASELINE config 5 wants to survive a restart) ----
    def SaveCheckpoint(self, path: str):
        """The running mean and the counters that index the frame sequence -> one .npz (readback submits and waits)."""
        np.savez(path, converged=self._converged.GetPixels(), currentSample=self._currentSample, frame=self._frame,
                 frame_seed=self.frame_seed, size=(self.screen_width, self.screen_height))

    def LoadCheckpoint(self, path: str):
        """Resume: the next OnRenderImage blends frame `frame` with alpha 1 / (currentSample + 1) into the restored mean."""
        z = np.load(path, allow_pickle=False)
        w, h = (int(v) for v in z["size"])
        if (w, h) != (self.screen_width, self.screen_height):
            raise ValueError("checkpoint is of another resolution")
        if self._treesNeedRebuilding:                       # RM:850-859 would reset the sample counter: do the rebuild first
            self._treesNeedRebuilding = False
            if self._rayTraceObjects:
                self.RebuildObjectLists()
            self.RebuildTrees()
        self.InitRenderTexture()
        self._converged.SetPixels(z["converged"])
        self._currentSample, self._frame, self.frame_seed = int(z["currentSample"]), int(z["frame"]), int(z["frame_seed"])

    # RM:188-212
    def OnDisable(self):
        if self.device_object_heaps:                                              # the scene's lists outlive the buffers
            self.SyncObjectHeaps()
        self.SyncGeometry()
        for b in (self._sphereBuffer, self._meshObjectBuffer, self._vertexBuffer, self._indexBuffer, self._normalBuffer,
                  self._sphereBVHBuffer, self._meshObjectBVHBuffer) + tuple(self._skinBuffers or ()) + tuple(self._boneBuffers.values()) \
                + tuple(self._leafBuffers):
            if b is not None:
                b.Release()
        self._skinBuffers, self._boneBuffers = None, {}
        self._leafBuffers, self._heapsBehind = [None, None], [False, False]
        self._drop_morphs()
        self._drop_normals_plans()
        for t in (self._target, self._converged, self.SkyboxTexture, self._denoised, self._tonemapped) + (self._aov or ()):
            if t is not None:
                t.Release()
        self._target = self._converged = self.SkyboxTexture = self._denoised = self._tonemapped = None
        self._aov = None
        self._release_upscale()
        self._release_temporal()
        self._release_dof()

    # ---- multi-GPU frame-end gather (no counterpart in the reference: it is single-GPU) -----------
    def gather_converged(self, dist, device):
        """One collective at frame end: every rank packs its strips of `_converged` into a dense device buffer
        (k_pack_rows), rank 0 gathers (RCCL; with the gloo backend the buffers are staged through host memory) and
        de-interleaves (k_pack_rows, reverse).  Returns the full image on rank 0 (numpy), else None.
        Synchronous by design (a convenience for tests and tools; bench.py pipelines the same steps on streams)."""
        import torch
        from . import strips
        from ._lib import UrtError
        if self._converged is None or not self._converged.handle:
            raise UrtError(2, "gather_converged: no accumulated image yet (render a frame first)")
        n_floats = strips.packed_rows(self.screen_height, self.world_size) * self.screen_width * 4
        mine = torch.zeros(n_floats, dtype=torch.float32, device=device)
        if mine.is_cuda:
            # the zero fill runs on torch's current stream, the pack kernel on the library's own stream: order them
            torch.cuda.current_stream(device).synchronize()
        self._converged.pack_rows(self.rank, self.world_size, mine.data_ptr())
        self.ctx.synchronize()
        staged = dist.get_backend() == "gloo"
        parts = strips.gather_to_root(dist, mine.cpu() if staged else mine, self.rank, self.world_size)
        if mine.is_cuda:
            torch.cuda.synchronize(device)
        if self.rank != 0:
            return None
        full = RenderTexture(self.ctx, self.screen_width, self.screen_height)
        keep = []
        for r, p in enumerate(parts):
            pd = p.to(device) if staged else p
            keep.append(pd)
            if pd.is_cuda:
                torch.cuda.current_stream(device).synchronize()             # the upload (torch's stream) before the unpack (library's stream)
            full.unpack_rows(r, self.world_size, pd.data_ptr())
        out = full.GetPixels()                                             # synchronises
        full.Release()
        return out
