"""The boundary traffic of RayTraceMaster, recorded: a real RayTraceMaster and the real unity_api wrappers drive a recording stand-in for
the ctypes library (the _StubLib / stub_context() idea of the test_*_abi.py files, for every entry point the master reaches), and
the list of calls that arrive there is the result.  No GPU, no kernel: the pixel tests cannot see a dropped SetShaderParameters or two
calls in another order that happen to render the same image; this can.

A record is [entry point, argument, ...]: handles as creation-order labels ("B3": the fourth buffer made, "T0", "N0" / "M0": plans; None
for a zero handle), ints as they are, floats as float.hex(), names as strings, structs as {field: value}, host arrays as "@k", an index
into the table of {shape, dtype, sha256} the trace comes with.  No pointer value and no id() is recorded.  ["#", text] records mark the
steps of the script.  The stand-in fills out-parameters deterministically (handles, urt_buffer_bounds, urt_resample_below's count, the
read-back of SyncObjectHeaps, one ray-query hit).

The script (run(): once with temporal accumulation off, once on, once on registered objects) is in script() below.  Auto-exposure needs
a tensor on a device: EnableAutoExposure is left out and an opaque state the stand-in accepts is injected into the two attributes it
sets, so that ToneMap's metering call is in the trace.

The expected trace, tests/golden/master_call_trace.json, is made from the commit BEFORE a refactoring of ray_trace_master.py /
unity_api.py, never from the refactored code:

    python tests/master_trace.py tests/golden/master_call_trace.json

To check the committed file: put that commit's unityraytracer_amd/ray_trace_master.py and unityraytracer_amd/unity_api.py over a
scratch copy of the tree (built) and run the command there; the output is byte-identical.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from unityraytracer_amd import RayTraceMaster, RayTraceObject, _lib, scenes, unity_api  # noqa: E402
from unityraytracer_amd._lib import UrtError  # noqa: E402

F = np.float32
WIDTH, HEIGHT = 16, 8

# entry points whose arguments need nothing but their kind: c = the context (not recorded), h = a handle, i = an int, f = a float,
# s = a name, S = a struct by reference, p = a device pointer ("state" or None)
SIMPLE = {
    "urt_buffer_copy": "chihii", "urt_buffer_release": "ch", "urt_texture_release": "ch",
    "urt_skin_vertices": "cSiihh", "urt_compute_normals": "chh", "urt_normals_plan_release": "ch",
    "urt_morph_vertices": "chhhhhhi", "urt_morph_plan_release": "ch",
    "urt_mesh_leaf_bounds_device": "chhhh", "urt_sphere_leaf_bounds_device": "chh", "urt_build_object_bvh_device": "chh",
    "urt_shader_set_buffer": "cish", "urt_shader_set_texture": "cish", "urt_shader_set_float": "csf", "urt_shader_set_int": "csi",
    "urt_shader_dispatch": "ciiii", "urt_blit_add": "chhf", "urt_blit": "chh", "urt_blit_add_history": "chhhf",
    "urt_render_aov": "chhhhi", "urt_denoise": "chhhhhS", "urt_reproject": "cSS", "urt_reproject_objects": "cSSS",
    "urt_reproject_deformed": "cSSSS", "urt_upsample": "cSS", "urt_auto_exposure": "chhSp", "urt_tonemap": "chhSp",
    "urt_depth_of_field": "chhhS", "urt_bloom": "chhSp",
}
CUSTOM = ("urt_buffer_create", "urt_buffer_set_data", "urt_buffer_set_data_range", "urt_buffer_get_data_range", "urt_buffer_bounds",
          "urt_normals_plan_create", "urt_morph_plan_create", "urt_texture_create", "urt_texture_set_pixels", "urt_shader_set_matrix",
          "urt_shader_set_vector", "urt_ray_query", "urt_radiance_query", "urt_resample_below")
# every entry point the master can reach through the methods of script(): the test wants each of them in the trace
REACHABLE = tuple(sorted(SIMPLE)) + CUSTOM
# the fields of the structs that hold handles
HANDLE_FIELDS = {"ReprojectImages": None, "UpsampleImages": None, "SkinBuffers": None,                 # None: all of them
                 "ReprojectMotion": ("mesh_motion", "sphere_motion"),
                 "ReprojectDeform": ("prev_vertices", "indices", "prev_mesh_objects", "deformed")}
REPROJECTS = ("urt_reproject", "urt_reproject_objects", "urt_reproject_deformed")


class RecordingLib:
    def __init__(self, arrays):
        self.trace = []
        self.arrays = arrays                                   # (shape, dtype, sha256) -> index, shared by the runs of one trace
        self.labels = {}                                       # handle -> label
        self.made = {"B": 0, "T": 0, "N": 0, "M": 0}
        self.strides, self.sizes = {}, {}                      # buffer handle -> stride; texture handle -> (width, height)

    def mark(self, text):
        self.trace.append(["#", text])

    # ---- how an argument is written down ----
    def _new(self, kind, out):
        handle = sum(self.made.values()) + 1
        self.labels[handle] = f"{kind}{self.made[kind]}"
        self.made[kind] += 1
        out._obj.value = handle
        return handle

    def _h(self, handle):
        handle = getattr(handle, "value", handle)
        return self.labels[handle] if handle else None

    @staticmethod
    def _f(v):
        return float(v).hex()

    def _array(self, ptr, shape, dtype):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        address = getattr(ptr, "value", ptr)
        data = C.string_at(address, nbytes) if nbytes and address else b""
        key = (tuple(int(n) for n in shape), np.dtype(dtype).name, hashlib.sha256(data).hexdigest())
        return f"@{self.arrays.setdefault(key, len(self.arrays))}"

    def _struct(self, ref):
        s = ref._obj
        handles = HANDLE_FIELDS.get(type(s).__name__, ())
        out = {}
        for name, _ in s._fields_:
            v = getattr(s, name)
            if handles is None or name in handles:
                out[name] = self._h(v)
            elif isinstance(v, C.Array):
                out[name] = self._array(C.addressof(v), (len(v),), F)      # (float arrays are the only ones)
            else:
                out[name] = self._f(v) if isinstance(v, float) else int(v)
        return out

    def __getattr__(self, name):
        kinds = SIMPLE.get(name)
        if kinds is None:
            raise AttributeError(name)
        how = {"h": self._h, "i": int, "f": self._f, "s": bytes.decode, "S": self._struct,
               "p": lambda p: "state" if getattr(p, "value", p) else None}

        def call(*args):
            assert len(args) == len(kinds), (name, len(args))
            self.trace.append([name] + [how[k](a) for k, a in zip(kinds, args) if k != "c"])
            if name.endswith("_release"):
                del self.labels[args[1]]                       # a released handle must not arrive again
            return 0
        return call

    # ---- the entry points that read host memory or fill an out-parameter ----
    def urt_buffer_create(self, ctx, count, stride, out):
        self.strides[self._new("B", out)] = stride
        self.trace.append(["urt_buffer_create", count, stride])
        return 0

    def urt_buffer_set_data(self, ctx, handle, data, n):
        self.trace.append(["urt_buffer_set_data", self._h(handle), self._array(data, (n, self.strides[handle]), np.uint8), n])
        return 0

    def urt_buffer_set_data_range(self, ctx, handle, first, data, count):
        self.trace.append(["urt_buffer_set_data_range", self._h(handle), first, self._array(data, (count, self.strides[handle]), np.uint8), count])
        return 0

    def urt_buffer_get_data_range(self, ctx, handle, first, out, count):
        self.trace.append(["urt_buffer_get_data_range", self._h(handle), first, count])
        fill = ((np.arange(count * self.strides[handle]) * 7 + first) % 256).astype(np.uint8).tobytes()
        C.memmove(out.value, fill, len(fill))
        return 0

    def urt_buffer_bounds(self, ctx, handle, first, count, out, n):
        self.trace.append(["urt_buffer_bounds", self._h(handle), first, count])
        box = np.array([-1.0 - first / 16.0] * 3 + [1.0 + count / 16.0] * 3, dtype=F).tobytes()
        C.memmove(out.value, box, len(box))
        n._obj.value = count
        return 0

    def urt_normals_plan_create(self, ctx, vertices, indices, first, count, out):
        self._new("N", out)
        self.trace.append(["urt_normals_plan_create", self._h(vertices), self._h(indices), first, count])
        return 0

    def urt_morph_plan_create(self, ctx, deltas, n, n_targets, first, count, out):
        self._new("M", out)
        self.trace.append(["urt_morph_plan_create", self._array(deltas, (n, 32), np.uint8), n, n_targets, first, count])
        return 0

    def urt_texture_create(self, ctx, width, height, out):
        self.sizes[self._new("T", out)] = (width, height)
        self.trace.append(["urt_texture_create", width, height])
        return 0

    def urt_texture_set_pixels(self, ctx, handle, data):
        w, h = self.sizes[handle]
        self.trace.append(["urt_texture_set_pixels", self._h(handle), self._array(data, (h, w, 4), F)])
        return 0

    def urt_shader_set_matrix(self, ctx, name, data):
        self.trace.append(["urt_shader_set_matrix", name.decode(), self._array(data, (16,), F)])
        return 0

    def urt_shader_set_vector(self, ctx, name, packed):
        self.trace.append(["urt_shader_set_vector", name.decode(), [self._f(x) for x in np.frombuffer(packed, dtype=F)]])
        return 0

    def urt_ray_query(self, ctx, rays, n, out, flags):
        self.trace.append(["urt_ray_query", self._array(rays, (n, 32), np.uint8), n, flags])
        hit = np.zeros(n, dtype=unity_api.RAYHIT_DT)
        hit["distance"], hit["kind"], hit["normal"] = 2.0, 1, (0.0, 1.0, 0.0)
        C.memmove(out.value, hit.tobytes(), hit.nbytes)
        return 0

    def urt_radiance_query(self, ctx, queries, n, samples, bounces, out, flags):
        stride = _lib.URT_STRIDE_PATHPIXEL if flags == _lib.URT_RADIANCE_PIXELS else _lib.URT_STRIDE_PATHRAY
        self.trace.append(["urt_radiance_query", self._array(queries, (n, stride), np.uint8), n, samples, bounces, flags])
        return 0

    def urt_resample_below(self, ctx, dst, count, below, samples, bounces, weight, max_history, n):
        self.trace.append(["urt_resample_below", self._h(dst), self._h(count), self._f(below), samples, bounces, self._f(weight),
                           self._f(max_history)])
        n._obj.value = 3
        return 0


class _Device:
    type, index = "cuda", 0


class _StateTensor:
    """What the wrappers ask of an exposure state (a torch tensor on the device), without a device."""
    __module__ = "torch.stub"
    device = _Device()

    def data_ptr(self):
        return 0x7000

    def numel(self):
        return 260

    def element_size(self):
        return 4

    def is_contiguous(self):
        return True


def stub_context(lib):
    ctx = object.__new__(unity_api.Context)
    ctx.lib, ctx._h, ctx.device = lib, C.c_void_p(1), 0
    return ctx


def scene():
    """mixed_test_scene: three meshes (a blob, an icosphere, a quad) and five spheres, with a constant sky."""
    return scenes.mixed_test_scene(WIDTH, HEIGHT, sky=np.full((2, 4, 4), 0.5, F))


def camera(k, w=WIDTH, h=HEIGHT):
    return scenes.camera_matrices(w, h, position=(0.25 * k, 1.0 + 0.125 * k, -10.0))


def bones(k, n=2):
    b = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F), (n, 1))
    b[:, 9:] = np.arange(n, dtype=F)[:, None] * 0.125 + 0.0625 * k
    return b


def attach(m):
    """A skin on mesh 0, blend shapes on mesh 1, both on mesh 2 (on the same span)."""
    s = m.scene
    for k in (0, 2):
        lo, hi = m.vertex_span(k)
        idx, wgt = np.zeros((hi - lo + 1, 4), np.int32), np.zeros((hi - lo + 1, 4), F)
        idx[:, 1], wgt[:, 0], wgt[:, 1] = 1, 0.75, 0.25
        m.AttachSkin(k, idx, wgt)
    for k in (1, 2):
        lo, hi = m.vertex_span(k)
        v = np.asarray(s.vertices, F).reshape(-1, 3)[lo: hi + 1]
        sparse = v * F(0.125)
        sparse[1::2] = 0
        m.AttachBlendShapes(k, [(v * F(0.25), None), (sparse, -sparse)])


def positions(m, k, scale):
    lo, hi = m.vertex_span(k)
    return np.asarray(m.scene.vertices, F).reshape(-1, 3)[lo: hi + 1] * F(scale)


def frames(m, n=2, destination=None):
    for _ in range(n):
        m.OnRenderImage(destination)


def edits(m, mark, tag, k):
    """One call of every form of the four edits (MoveCamera, MoveObjects, DeformMeshes, SkinMeshes / MorphMeshes), frames in between."""
    c2w, invp = camera(k)
    mark(f"MoveCamera {tag}")
    m.MoveCamera(c2w)
    frames(m, 1)
    mark(f"MoveCamera {tag} projection")
    m.MoveCamera(camera(k + 1)[0], invp)
    frames(m, 1)
    mesh = {0: scenes.trs(translate=(-2.0 + 0.125 * k, 1.3, 1.0), yaw_deg=10.0 * k)}
    sphere = {1: ((0.5 * k, 1.0, 2.0), 0.75), 3: ((-1.0, 0.5 + 0.125 * k, 0.0), 0.5)}
    for what, kw in (("mesh", {"mesh_edits": mesh}), ("sphere", {"sphere_edits": sphere}),
                     ("both", {"mesh_edits": {1: scenes.trs(translate=(2.5, 1.0 + 0.125 * k, -1.0)), 2: scenes.trs()}, "sphere_edits": {0: ((3.0, 1.0, 0.5 * k), 1.0)}}),
                     ("camera", {"mesh_edits": mesh, "camera_to_world": camera(k + 2)[0], "camera_inverse_projection": invp}),
                     ("nothing", {})):
        mark(f"MoveObjects {tag} {what}")
        m.MoveObjects(**kw)
        frames(m, 1)
    for what, args in (("normals", ({1: positions(m, 1, 1.0625)}, True, False)), ("positions", ({1: positions(m, 1, 0.9375)}, False, False)),
                       ("normals keep", ({0: positions(m, 0, 1.03125), 2: positions(m, 2, 1.0)}, True, True)),
                       ("positions keep", ({2: positions(m, 2, 0.984375)}, False, True)), ("nothing keep", ({}, True, True))):
        mark(f"DeformMeshes {tag} {what}")
        m.DeformMeshes(*args)
        frames(m, 1)
    for what, args in (("plain", ({0: bones(k)}, False, False)), ("normals", ({0: bones(k + 1), 2: bones(k, 3)}, True, False)),
                       ("keep", ({2: bones(k + 2)}, False, True)), ("normals keep", ({0: bones(k + 3)}, True, True)), ("nothing", ({}, False, True))):
        mark(f"SkinMeshes {tag} {what}")
        m.SkinMeshes(*args)
        frames(m, 1)
    w1, w2 = np.array([0.5, 0.25 * k], F), np.array([1.0, -0.5], F)
    for what, args in (("plain", ({1: w1}, None, False, False)), ("poses", ({1: w1, 2: w2}, {2: bones(k)}, False, False)),
                       ("poses normals", ({2: w1}, {2: bones(k + 1)}, True, False)), ("normals keep", ({1: w2, 2: w2}, None, True, True)),
                       ("poses keep", ({1: w1, 2: w1}, {2: bones(k + 2)}, False, True))):
        mark(f"MorphMeshes {tag} {what}")
        m.MorphMeshes(*args)
        frames(m, 1)


def device_side(m, mark, tag, k):
    """The paths that can build the object-level heaps on the device, with the flag set."""
    m.device_object_heaps = True
    for what, kw in (("mesh", {"mesh_edits": {1: scenes.trs(translate=(2.5, 1.5, -1.0 + 0.25 * k))}}), ("sphere", {"sphere_edits": {2: ((1.0, 2.0, 0.25 * k), 0.5)}}),
                     ("both", {"mesh_edits": {0: scenes.trs(translate=(-2.0, 1.0, 1.0))}, "sphere_edits": {4: ((0.0, 1.0, -2.0), 0.25)},
                               "camera_to_world": camera(k)[0]})):
        mark(f"MoveObjects {tag} device heaps {what}")
        m.MoveObjects(**kw)
        frames(m, 1)
    mark(f"SkinMeshes {tag} device heaps")
    m.SkinMeshes({0: bones(k + 4)}, False, True)
    mark(f"MorphMeshes {tag} device heaps")
    m.MorphMeshes({1: np.array([0.125, 0.5], F), 2: np.array([0.0, 1.0], F)}, {2: bones(k + 5)}, True, False)
    mark(f"SyncObjectHeaps {tag} spheres")
    m.SyncObjectHeaps(meshes=False)
    mark(f"SyncObjectHeaps {tag}")
    m.SyncObjectHeaps()
    frames(m, 1)
    mark(f"MoveObjects {tag} device heaps, then a rebuild")
    m.MoveObjects(mesh_edits={2: scenes.trs(translate=(0.0, 0.125, 0.0))}, sphere_edits={0: ((3.0, 1.0, 0.0), 1.0)})
    m._treesNeedRebuilding = True                              # (what RegisterObject sets)
    frames(m, 2)
    m.device_object_heaps = False


def image_space(m, mark, tag, temporal):
    ctx = m.ctx
    mark(f"RecomputeNormals {tag}")
    m.RecomputeNormals()
    m.RecomputeNormals([1])
    mark(f"Raycast {tag}")
    assert m.Raycast((0.0, 1.0, -10.0), (0.0, 0.0, 1.0))["kind"] == 1
    m.Raycast((0.0, 1.0, -10.0), (0.0, 1.0, 0.0), 5.0)
    mark(f"SampleRadiance, ResamplePixels {tag}")
    m.SampleRadiance(np.zeros((3, 3), F), np.tile(np.array([0, 0, 1], F), (3, 1)), 2)
    m.ResamplePixels(np.array([[0, 0], [3, 2]], np.int32))
    mark(f"RenderFeatureBuffers {tag}")
    m.RenderFeatureBuffers()
    m.RenderFeatureBuffers(frame_ray=True)
    mark(f"Denoise {tag}")
    m.Denoise()
    m.Denoise(unity_api.RenderTexture(ctx, m.screen_width, m.screen_height), iterations=2, sigma_color=4.0)
    mark(f"Upscale {tag}")
    w, h = 2 * m.screen_width, 2 * m.screen_height
    m.Upscale(w, h)
    m.Upscale(w, h, fill_holes=True, below=1.5, normal_threshold=0.5)
    m.Upscale(w, h, unity_api.RenderTexture(ctx, w, h), wide_fallback=False)
    m.Upscale(w + 8, h)                                        # another presented size: the textures are made anew
    mark(f"ResampleDisocclusions {tag}")
    if temporal:
        assert m.ResampleDisocclusions() == 3
        m.ResampleDisocclusions(2.0)
    else:
        try:
            m.ResampleDisocclusions()
            raise AssertionError("ResampleDisocclusions without temporal accumulation went through")
        except UrtError:
            pass
    mark(f"ToneMap {tag}")
    m.ToneMap()
    m.ToneMap(unity_api.RenderTexture(ctx, m.screen_width, m.screen_height), "reinhard", 2.0, 8.0)
    for what, on in (("bloom", (0, 1, 0)), ("bloom, depth of field", (0, 1, 1)), ("depth of field", (0, 0, 1)), ("exposure", (1, 0, 0)),
                     ("exposure, bloom, depth of field", (1, 1, 1)), ("all off again", (0, 0, 0))):
        mark(f"ToneMap {tag} {what}")
        m._exposure, m._exposureState = ({"key": 0.25, "rate": 0.5}, _StateTensor()) if on[0] else (None, None)   # (EnableAutoExposure: see above)
        m.EnableBloom(threshold=1.5, levels=3) if on[1] else m.DisableBloom()
        m.EnableDepthOfField(focus_distance=9.0, scale=4.0) if on[2] else m.DisableDepthOfField()
        m.ToneMap()
        m.ToneMap(unity_api.RenderTexture(ctx, m.screen_width, m.screen_height), "linear")
    frames(m, 1, unity_api.RenderTexture(ctx, m.screen_width, m.screen_height))


def resize(m, mark, tag, temporal):
    """The screen changes size: every call that owns a texture makes it anew."""
    m.screen_width, m.screen_height = WIDTH + 8, HEIGHT + 8
    c2w, invp = camera(7, m.screen_width, m.screen_height)
    mark(f"MoveCamera {tag} after a resize")
    m.MoveCamera(c2w, invp)                                    # _converged still has the old size: no history
    frames(m, 2)
    m.EnableBloom()
    m.EnableDepthOfField()
    mark(f"owned textures {tag} after a resize")
    m.RenderFeatureBuffers()
    m.Denoise()
    m.Upscale(2 * m.screen_width, 2 * m.screen_height, fill_holes=True)
    m.ToneMap()
    if temporal:
        m.ResampleDisocclusions()
    m.screen_width, m.screen_height = WIDTH, HEIGHT
    frames(m, 1)
    mark(f"Denoise, ToneMap {tag} after the next resize")
    m.Denoise()                                                # (the feature buffers still have the other size)
    m.ToneMap()
    m.DisableBloom()
    m.DisableDepthOfField()
    mark(f"MoveObjects {tag} after the resize")
    m.MoveObjects(sphere_edits={0: ((2.0, 1.0, 0.0), 1.0)}, camera_to_world=camera(8)[0], camera_inverse_projection=camera(8)[1])
    mark(f"DeformMeshes {tag} after the resize")
    m.DeformMeshes({1: positions(m, 1, 1.0)}, keep_history=True)
    mark(f"SkinMeshes {tag} after the resize")
    m.SkinMeshes({0: bones(9)}, keep_history=True)


def needing_a_rebuild(m, mark, tag, flag):
    """One call of each edit on a master whose trees still need rebuilding (flag() sets that again where a call has made them)."""
    mark(f"MoveCamera {tag} before the trees exist")
    m.MoveCamera(camera(1)[0])
    mark(f"MoveObjects {tag} before the trees exist")
    m.MoveObjects(mesh_edits={0: scenes.trs(translate=(-2.0, 1.25, 1.0))}, sphere_edits={0: ((1.0, 1.0, 1.0), 0.5)})
    mark(f"DeformMeshes {tag} before the trees exist")
    m.DeformMeshes({1: positions(m, 1, 1.015625)})
    mark(f"SkinMeshes {tag} before the trees exist")
    m.SkinMeshes({0: bones(0)})
    flag()
    mark(f"MorphMeshes {tag} before the trees exist")
    m.MorphMeshes({1: np.array([0.5, 0.5], F)}, keep_history=True)
    flag()
    mark(f"RecomputeNormals, Raycast, RenderFeatureBuffers {tag} before the trees exist")
    m.RecomputeNormals([0])
    flag()
    m.Raycast((0.0, 1.0, -10.0), (0.0, 0.0, 1.0))
    flag()
    m.RenderFeatureBuffers()
    flag()


def script(temporal):
    """The whole script on the pre-flattened scene."""
    def run(lib):
        tag = "temporal" if temporal else "plain"
        m = RayTraceMaster(stub_context(lib), scene())
        attach(m)
        if temporal:
            lib.mark("EnableTemporalAccumulation")
            m.EnableTemporalAccumulation(moved_max_history=8.0)

        def flag():
            m._treesNeedRebuilding = True                      # (what RegisterObject sets)
        needing_a_rebuild(m, lib.mark, tag, flag)
        frames(m, 2)
        edits(m, lib.mark, tag, 1)
        device_side(m, lib.mark, tag, 2)
        image_space(m, lib.mark, tag, temporal)
        resize(m, lib.mark, tag, temporal)
        if temporal:
            lib.mark("EnableTemporalAccumulation with a deform threshold")
            m.EnableTemporalAccumulation(max_history=16.0, deform_normal_threshold=0.25)
            frames(m, 2)
            lib.mark("DeformMeshes temporal threshold keep")
            m.DeformMeshes({1: positions(m, 1, 1.0)}, keep_history=True)
            lib.mark("MorphMeshes temporal threshold keep")
            m.MorphMeshes({1: np.array([0.0, 0.0], F)}, keep_history=True)
            lib.mark("DisableTemporalAccumulation")
            m.DisableTemporalAccumulation()
            frames(m, 1)
            lib.mark("MoveCamera plain again")
            m.MoveCamera(camera(3)[0])
        lib.mark("OnDisable")
        m.OnDisable()
    return run


def registered(lib):
    """Registered objects (RegisterObject) instead of a pre-flattened scene: the other source of the host's object-level heaps."""
    sc = scene()
    m = RayTraceMaster(stub_context(lib), sc)
    v = np.asarray(sc.vertices, F).reshape(-1, 3)
    for k, mo in enumerate(sc.mesh_objects):
        first, n = int(mo["indices_offset"]), int(mo["indices_count"])
        tri = np.asarray(sc.indices[first: first + n])
        m.RegisterObject(RayTraceObject(type=0, vertices=v[tri.min(): tri.max() + 1], triangles=tri - tri.min(),
                                        localToWorldMatrix=np.array(mo["localToWorldMatrix"], F), smoothness=0.25 * k))
    for sp in sc.spheres[:2]:
        m.RegisterObject(RayTraceObject(type=1, position=tuple(float(x) for x in sp["position"]), radius=float(sp["radius"])))
    attach(m)
    lib.mark("EnableTemporalAccumulation registered")
    m.EnableTemporalAccumulation()

    def flag():
        m.RegisterObject(RayTraceObject(type=1, position=(0.0, 3.0, 0.0), radius=0.25))
    needing_a_rebuild(m, lib.mark, "registered", flag)
    frames(m, 2)
    lib.mark("MoveObjects registered both")
    m.MoveObjects(mesh_edits={1: scenes.trs(translate=(2.0, 1.0, -1.0))}, sphere_edits={1: ((0.0, 1.0, 0.0), 0.5)})
    lib.mark("DeformMeshes registered normals")
    m.DeformMeshes({0: positions(m, 0, 1.0625)}, True, True)
    lib.mark("SkinMeshes registered")
    m.SkinMeshes({0: bones(1), 2: bones(2)})
    lib.mark("MorphMeshes registered")
    m.MorphMeshes({2: np.array([0.5, 0.5], F)}, {2: bones(3)})
    m.device_object_heaps = True
    lib.mark("MoveObjects registered device heaps sphere")
    m.MoveObjects(sphere_edits={0: ((1.0, 1.0, 0.0), 0.5)})
    lib.mark("SkinMeshes registered device heaps")
    m.SkinMeshes({0: bones(4)})
    lib.mark("OnDisable registered")
    m.OnDisable()


RUNS = (("plain", script(False)), ("temporal", script(True)), ("registered", registered))


def run():
    """{"arrays": the table the "@k" of the records index, "runs": {name: [record, ...]}}"""
    arrays, runs = {}, {}
    sync, unity_api._sync_torch_stream = unity_api._sync_torch_stream, lambda t: None      # (no torch stream behind the opaque state)
    try:
        for name, body in RUNS:
            lib = RecordingLib(arrays)
            body(lib)
            runs[name] = lib.trace
    finally:
        unity_api._sync_torch_stream = sync
    return {"arrays": [{"shape": list(shape), "dtype": dtype, "sha256": digest} for shape, dtype, digest in arrays], "runs": runs}


def dumps(trace):
    """One line per record: a difference between two files reads as a difference between two call lists."""
    def lines(items):
        return ",\n".join(json.dumps(item, separators=(",", ":")) for item in items)
    runs = ",\n".join(f"{json.dumps(name)}:[\n{lines(records)}\n]" for name, records in trace["runs"].items())
    return f'{{"arrays":[\n{lines(trace["arrays"])}\n],\n"runs":{{\n{runs}\n}}}}\n'


def branches(records):
    """{edit: {True, False}}: whether the calls of each edit, found by their step marks, reprojected (history kept) or did not."""
    taken, edit = {}, None
    for r in records:
        if r[0] == "#":
            edit = next((e for e in ("MoveCamera", "MoveObjects", "DeformMeshes", "SkinMeshes", "MorphMeshes") if r[1].startswith(e + " ")), None)
            if edit is not None:
                step = [edit, False]
                taken.setdefault(edit, []).append(step)
        elif edit is not None and r[0] in REPROJECTS:
            step[1] = True
    return {e: {kept for _, kept in steps} for e, steps in taken.items()}


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        f.write(dumps(run()))
