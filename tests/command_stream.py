"""Random command streams, a sequential model of them, and a runner (no GPU needed to import; tests/test_command_stream_model.py,
tests/test_gpu_command_stream.py).

The library defers: dispatches wait in a batch, the blends / presents behind them are queued, small launches alternate between two
trace streams behind a narrow dependency (csrc/frame_batch.cpp flush_pending).  The contract is PROGRAM ORDER: every call behaves as
if it ran alone, at once, on one stream.  A program here is a list of plain op tuples over a small fixed world; `run_model` executes it
sequentially with numpy arrays as textures and the oracle as the trace kernel, `run_gpu` executes it through the Python API.

The world: scenes.mixed_test_scene(width, height) with `bounces` bounces and one ray, ONE RayTraceMaster, and these textures:
    T0, T1      the two Result textures (the master's _target is one of them; "bind_result" swaps — to the library that is what a
                second camera's _target is: another Result texture under the same bindings)
    C           the master's _converged
    X0, X1, X2  frame-sized extras (present destinations, blit partners)
    H, N        a history / count pair for blit_add_history
    S0, S1      the scene's own sky and another texture of its size
Ops (first element = kind):
    ("frame", dest | None)             OnRenderImage(dest): dispatch, additive blend into C, optional present
    ("dispatch", "T0" | "T1")          bare dispatch into that Result texture, no blend (advances the frame sequence)
    ("blit", src, dst)                 Graphics.Blit between two textures of one size
    ("history", max_history)           ctx.blit_add_history(_target, H, N, max_history)
    ("setpixels", tex, value)          SetPixels(constant)
    ("restart",)                       _currentSample = 0
    ("bind_sky", tex | None)           _SkyboxTexture = tex (reaches the library at once)
    ("bind_result",)                   the master's _target becomes the other Result texture
    ("move_mesh", k, j)                SetData of _MeshObjects with object k at MOVES[j], and of the rebuilt heap
    ("deform", scale)                  ranged SetData of the blob's vertices scaled about their centre, and of the rebuilt heap
    ("move_spheres", j)                SetData of _Spheres shifted by SHIFTS[j], and of the rebuilt heap
    ("camera", j)                      _CameraToWorld = CAMERAS[j]
    ("flush",)                         ctx.flush()
    ("ptr", tex)                       device_ptr() (pointer hand-out: the image is never renamed again)
    ("get", tex)                       observer: GetPixels
    ("read_begin", tex, fmt)           observer: ReadBegin (at most two tickets in flight); observed at the matching
    ("read_end",)                      ... ReadEnd of the oldest ticket
    ("ray_query", seed)                observer: 64 closest-hit queries
    ("radiance_query", seed)           observer: 64 radiance queries (recorded, not modelled: compared between configurations only)
A dispatch never runs while its own Result texture is bound as the sky (a kernel that samples the image it writes has no sequential
meaning, in Unity neither), and blit_add_history never while H or N is the sky (the library refuses it): the generator keeps to that.

The "pipeline" profile (make_program(seed, profile="pipeline"), run_model / run_gpu with profile="pipeline") adds the image-space and
device-side calls around the frame loop.  More frame-sized textures: two feature-buffer sets Gh Gn Ga Gi and Ph Pn Pa Pi (hit, normal,
albedo, id), R / RN / MV (reprojected colour, count and the motion image) and D (the denoised image).  Buffers: V = _Vertices, NB =
_Normals, SNAP (a snapshot of V), the blob's rest pose, bone indices and weights, one bone table per pose of POSE_ANGLES, and one
NormalsPlan of the blob's span made at the start.  Its ops, besides the ones above (radiance_query is modelled in this profile):
    ("aov", set, mask, frame_ray)      ctx.render_aov into the targets of set "G" | "P" chosen by the bits of mask (1 hit, 2 normal, 4 albedo, 8 id)
    ("aov_into", tex)                  ctx.render_aov(albedo=tex): any frame texture that is not the bound sky
    ("reproject", form, j, max_history, src)   ctx.reproject of src (C | H) and N from set P to set G into R / RN / MV; the previous
                                       camera is CAMERAS[j]; form "plain" | "objects" (motion tables between the scene at the last
                                       ("aov", "P", ...) and now) | "deformed" (the blob by per-vertex motion from SNAP, too)
    ("denoise", src, iterations, albedo)   ctx.denoise(src, D, Gh, Gn, Ga if albedo else None).  D is written by nothing else and read
                                       by observers only: tests/denoise_ref.py is float64, so the model holds D as float64 and `same`
                                       compares it within the bound include/urt.h states, 1e-4 (1 + |formula|); alpha bit for bit
    ("select", tex, below)             observer: ctx.select_pixels
    ("resample", below, samples, max_history)   ctx.resample_below(H, N, ...): observed is the number resampled
    ("radiance_pixels", seed)          observer: ctx.radiance_query_pixels of 64 pixels, one sample
    ("skin", pose, normals, first, count)   ctx.skin_vertices of that range of the blob into the device side of V (and NB), and SetData of the heap
    ("normals",)                       the NormalsPlan's compute(NB)
    ("set_device", first, count, scale)     V.SetDataDevice(torch tensor): the range scaled about its centre, and SetData of the heap
    ("set_host", first, count, scale)       the same through the ranged host SetData (V has a mirror: the upload ring)
    ("snapshot",)                      SNAP.CopyFrom(V)
    ("get_buffer", which, first, count)     observer: GetData of V | NB | SNAP
    ("bounds", first, count)           observer: ctx.buffer_bounds(V, first, count)
    ("ray_query_async", seed) / ("radiance_async", seed)   the device entry points on torch tensors, not waited for: observed (under the
                                       op's own index) just before the next op of OBSERVERS or at the end, after ctx.synchronize() —
                                       the model answers with the scene as it was at the call
The library refuses an output that is the bound sky or one of the call's inputs and resample_below while H or N is the sky.

The "display" profile (profile="display") adds the display calls to the pipeline profile: every op above, and guide-driven upsampling,
auto-exposure, tone mapping and bloom.  More textures: a LOW GRID, a third size class — Lc (colour), Ln (count), Lh, Lm (normal), Li
(id), low_size(width, height) = 24 x 16 under the 64 x 40 frame, so that neither ratio is an integer — and the frame-sized U / UN
(upsampled colour and count).  Two EXPOSURE STATES E0, E1: torch.zeros(260, dtype=torch.int32) on the context's device, in the model
the dict tests/tonemap_ref.py passes around; the master's own state is "MS" (it starts with EnableAutoExposure(rate=0.5)) and the
texture it owns "TM" (all zero until the first ToneMap without a destination makes it).  A state is observed and compared as
state_words: exposure and target as bits, counted, skipped and the 256 bins as integers.  Its ops:
    ("aov_low", frame_ray)             ctx.render_aov(Lh, Lm, Lc, Li): the albedo target doubles as the low colour
    ("upsample", color, count | None, with_low_count, flags)   ctx.upsample(Lc, Lh, Lm, Li, Gh, Gn, Gi, color, count, low_count=Ln if
                                       with_low_count, albedo=Ga if flags has SKY_FROM_ALBEDO); flags over WIDE_FALLBACK | SKY_FROM_ALBEDO
    ("meter", src, k, with_count, j)   ctx.auto_exposure(src, E_k, count=N if with_count, **METER[j]); src of any size class
    ("tonemap", src, dst, k | None, op, exposure)   ctx.tonemap(src, dst, E_k, op=op, exposure=exposure); dst may be src
    ("bloom", src, dst, k | None, levels, flags)    ctx.bloom(src, dst, E_k, levels=levels, flags=flags); dst may be src
    ("state_get", k)                   observer: ctx.exposure_state(E_k)
    ("state_reset", k)                 ctx.synchronize(); E_k.zero_() — see run_gpu: the wait is the caller's part of the contract
    ("master_bloom", on)               EnableBloom(**MASTER_BLOOM) | DisableBloom()
    ("present_tm", dest | None, operator)   m.ToneMap(dest, operator): meter C into MS, bloom C into dest with MS if bloom is on, tone-map
                                       with MS; None = the texture the master owns, "TM" to ("get", "TM") and in the final contents
The library refuses a tonemap / bloom destination that is the bound sky, textures of two sizes in one of these calls (upsample: within
either grid), a count image for a source of another size, and ToneMap into _converged.

The "dynamic" profile (profile="dynamic") adds blend shapes, the object-level heaps built on the device and depth of field to the
display profile: every op above, and the ones below.  More of the world (dynamic_world): a MorphPlan of three sparse targets over the
blob's span (the rest pose is the skin ops'), the weights buffer W (stride 4) that the host rewrites in front of every morph, the leaf
buffers LM / LS (stride 28, one leaf per MeshObject / sphere), the names HM / HS for the two BOUND heap buffers (_MeshBVH / _SphereBVH), and
"DH", the hit guide the master owns once ToneMap has run with depth of field on (all zero until then).  Its ops:
    ("morph", j, with_normals, normalize)   W.SetData(MORPH_WEIGHTS[j]), plan.morph(rest_v, rest_n, W, V, NB | None, normalize) — the rest
                                       normals are passed exactly when NB is — and SetData of the heap, as the other vertex writes do
    ("device_heap", edit)              `edit` — an op of DEVICE_EDITS: SCENE_CHANGES without "normals", and "morph" — WITHOUT its host SetData of
                                       the heap; instead ctx.mesh_leaf_bounds(_MeshObjects, V, _Indices, LM), ctx.build_object_bvh(LM, HM), or
                                       the sphere pair for "move_spheres": three (two) kernels on the context's stream into the bound heap
                                       buffer's device side.  The model: host_scene.build_object_bvh(host_scene.mesh_leaf_bounds(...)) — the
                                       values the device computes, NOT scenes.mesh_bounds, which rounds outward
    ("rebuild_heap", kind)             the device build of kind 0 (meshes) | 1 (spheres) with no edit in front of it
    ("get_buffer", which, first, count)     also of HM | HS | LM | LS, observed as heap_words: 7 words per element
    ("dof", src, hit, dst, j)          ctx.depth_of_field(src, hit, dst, **DOF[j]): hit is Gh | Ph with frame-sized src / dst, or Lh with src /
                                       dst of the low grid
    ("master_dof", j | None)           EnableDepthOfField(**DOF[j]) | DisableDepthOfField(); while on, ("present_tm", ...) meters, renders the
                                       hit guide through the sample centres into DH, blurs C into the destination, blooms it in place if
                                       bloom is on and tone-maps it in place; the host's projection is bound again afterwards
The library refuses a depth-of-field destination that is the source, the hit image or the bound sky, textures of two sizes, normalize
without normals; the heap calls a destination that is also an input.

A second WORLD, world="solo" (make_scene, cameras, edited_scene, pipeline_world, dynamic_world, run_model, run_gpu; the default "mixed" is
everything above): the blob of the mixed scene alone — one MeshObject, no sphere, the same material, transform and sky — so that a trace
launch is the plain single-mesh form of the kernel, with the normal cones and the tile entry table.  The blob's span is the whole vertex
list; the skin, the morph targets, the normals plan and the rest pose are made from that span as in the mixed world.  Zero-count buffers
(sphere motion, LS, HS) do not exist in it.  The "solo" profile (profile="solo", which implies the world) is the dynamic profile without
the spheres' ops — no move_spheres, no rebuild_heap 1, no get_buffer of HS / LS, move_mesh of object 0 only, reproject form "objects"
with the mesh table only — and
    ("motion_blur", src, hit, dst, j)  ctx.motion_blur(src, MV, hit, dst, **MBLUR[j]): hit is Gh | Ph, src any exact frame-sized texture,
                                       dst any frame-sized texture but src, MV, hit and the bound sky (the library refuses those);
                                       played only once a reproject has written MV and an aov the hit set
run_gpu(options=...) sets tile_entry / refit / prepare_device for one run."""
import copy

import numpy as np

from unityraytracer_amd import scenes

F = np.float32
FRAME_TEX = ("T0", "T1", "C", "X0", "X1", "X2", "H", "N")
SKY_TEX = ("S0", "S1")
ALL_TEX = FRAME_TEX + SKY_TEX
FORMATS = ("RGBA32F", "RGBA8_SRGB", "RGBA16F")
KINDS = ("frame", "dispatch", "blit", "history", "setpixels", "restart", "bind_sky", "bind_result", "move_mesh", "deform", "move_spheres",
         "camera", "flush", "ptr", "get", "read_begin", "read_end", "ray_query", "radiance_query")
SUBMITTING = ("flush", "get", "read_begin", "setpixels", "ptr", "state_reset")   # ops that always submit the deferred frames themselves
WRITER_KINDS = ("blend", "history", "present", "blit", "dispatch", "setpixels")      # what can have written a texture last (coverage)
FRAME_SEED = 0x5EED
N_QUERIES = 64
MOVES = [dict(translate=(-1.2, 1.6, 0.4), scale=(1.2, 1.0, 0.9), yaw_deg=33.0),
         dict(translate=(-1.0, 1.5, 0.2), scale=(2.1, 0.45, 1.3), yaw_deg=-71.0),
         dict(translate=(-0.8, 1.7, 0.5), scale=(1.0, 1.0, 1.0), yaw_deg=10.0)]
SHIFTS = [(0.25, 0.0, -0.5), (-0.5, 0.25, 0.0), (0.0, -0.125, 0.75)]
CAMERA_POSITIONS = [(0.0, 1.0, -10.0), (1.5, 2.0, -9.0), (-2.0, 0.5, -11.0)]
DEFORM_SCALES = (0.75, 1.25, 0.9)
# the pipeline profile
G_TEX, P_TEX = ("Gh", "Gn", "Ga", "Gi"), ("Ph", "Pn", "Pa", "Pi")
PIPE_TEX = G_TEX + P_TEX + ("R", "RN", "MV", "D")
EXACT_TEX = FRAME_TEX + PIPE_TEX[:-1]                            # frame-sized textures that may be an input of anything (not D)
BUFFERS = ("V", "NB", "SNAP")
NEW_KINDS = ("aov", "aov_into", "reproject", "denoise", "select", "resample", "radiance_pixels", "skin", "normals", "set_device", "set_host",
             "snapshot", "get_buffer", "bounds", "ray_query_async", "radiance_async")
PIPE_KINDS = KINDS + NEW_KINDS
OBSERVERS = ("get", "read_end", "ray_query", "radiance_query", "select", "resample", "radiance_pixels", "get_buffer", "bounds", "state_get")
IMAGE_OPS = ("aov", "aov_into", "reproject", "denoise", "select", "resample")
VERTEX_WRITES = ("skin", "normals", "set_device", "set_host")    # in-place writes of V / NB (the last one through the host copy)
SCENE_CHANGES = ("move_mesh", "deform", "move_spheres") + VERTEX_WRITES
POSE_ANGLES = (25.0, -40.0, 60.0)
FORMS = ("plain", "objects", "deformed")
# the display profile
LOW_TEX = ("Lc", "Ln", "Lh", "Lm", "Li")                         # the low grid: colour, count, hit, normal, id
UP_TEX = ("U", "UN")
STATES = ("E0", "E1")
DISPLAY_FRAME_TEX = EXACT_TEX + UP_TEX
DISPLAY_EXACT = DISPLAY_FRAME_TEX + SKY_TEX + LOW_TEX            # what a display call may read: every texture but D
DISPLAY_KINDS = ("aov_low", "upsample", "meter", "tonemap", "bloom", "state_get", "state_reset", "master_bloom", "present_tm")
DISP_KINDS = PIPE_KINDS + DISPLAY_KINDS
DISPLAY_IMAGE_OPS = ("upsample", "meter", "tonemap", "bloom", "present_tm")
DISPLAY_WRITERS = ("upsample", "tonemap", "bloom")
WIDE_FALLBACK, SKY_FROM_ALBEDO, BLOOM_ONLY = 1, 2, 1             # URT_UPSAMPLE_WIDE_FALLBACK, _SKY_FROM_ALBEDO; URT_BLOOM_FLAG_ONLY
TONEMAP_OPS = ("linear", "reinhard", "aces")                     # in the order of URT_TONEMAP_*
METER = (dict(rate=1.0), dict(rate=0.25), dict(rate=0.5, key=0.25, low_permille=300, high_permille=800), dict(rate=0.5))
MASTER_EXPOSURE, MASTER_BLOOM = dict(rate=0.5), dict(levels=3)
STATE_WORDS = 260
# the dynamic profile
DYNAMIC_KINDS = ("morph", "device_heap", "rebuild_heap", "dof", "master_dof")
DYN_KINDS = DISP_KINDS + DYNAMIC_KINDS
DEVICE_EDITS = tuple(k for k in SCENE_CHANGES if k != "normals") + ("morph",)      # what ("device_heap", edit) wraps
HEAP_BUFFERS = ("HM", "HS", "LM", "LS")                          # the bound heaps and the leaves under them: stride 28
DYN_BUFFERS = BUFFERS + ("W",) + HEAP_BUFFERS
N_TARGETS = 3
MORPH_WEIGHTS = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.5), (0.5, -0.75, 0.0), (0.25, 0.5, 1.0))      # [0] all zero, [2] with a negative weight
DOF_FLAG_COC = 1                                                 # URT_DOF_FLAG_COC
# max_radius in each of the three reaches of csrc/dof.hip (<= 4, <= 8, <= 16).  [3] leaves the foreground sharp: from the first camera
# nothing is nearer than 1.56, and |scale * (1 - focus_distance / z)| <= 0.5 for every z in [1.36, 2.26] — each pixel nearer than 2.26 has
# the smallest blur radius and nothing in front of it is blurred, so its own tap is its only one (dof_foreground).  [4]: the blur radius
# instead of the image
DOF = (dict(focus_distance=3.0, scale=5.0, max_radius=4.0), dict(focus_distance=6.0, scale=9.0, max_radius=8.0),
       dict(focus_distance=2.25, scale=14.0, max_radius=16.0), dict(focus_distance=1.7, scale=2.0, max_radius=6.0),
       dict(focus_distance=10.0, scale=8.0, max_radius=8.0, flags=DOF_FLAG_COC))
DOF_IN_FOCUS = 3


def dof_foreground(hit):
    """The pixels DOF[DOF_IN_FOCUS] leaves bit for bit when nothing of the image is nearer than 1.36: those nearer than 2.26."""
    z = np.asarray(hit, F)[..., 3]
    assert not ((z > 0) & (z < F(1.36))).any(), "something lies in front of the in-focus band"
    return (z > 0) & (z < F(2.26))
DYNAMIC_IMAGE_OPS = DISPLAY_IMAGE_OPS + ("dof",)


def size_class(name):
    return 1 if name in SKY_TEX else 2 if name in LOW_TEX else 0


def low_size(width, height):
    """The low grid under a width x height frame: 24 x 16 under 64 x 40."""
    return width * 3 // 8, height * 2 // 5


def pyramid_texels(width, height, levels):
    """The texels of the levels urt_bloom keeps for a width x height image (include/urt.h "bloom": w_l = (w_{l-1} + 1) >> 1)."""
    import bloom_ref
    return sum(w * h for w, h in bloom_ref.level_sizes(width, height, levels))


def fresh_state():
    import tonemap_ref
    return dict(tonemap_ref.FRESH, hist=tonemap_ref.FRESH["hist"].copy())


def state_words(s):
    """An exposure state (the dict of tests/tonemap_ref.py and of Context.exposure_state) as the 260 words of urt_ExposureState:
    exposure and target as bits, counted, skipped and the bins as integers."""
    out = np.zeros(STATE_WORDS, np.uint32)
    out[:2] = np.array([s["exposure"], s["target"]], F).view(np.uint32)
    out[2], out[3] = s["counted"], s["skipped"]
    out[4:] = s["hist"]
    return out


# ---- the world ----------------------------------------------------------------------------------------------------------------------
WORLDS = ("mixed", "solo")
SOLO_BLOB = (20, 15)                                             # slices, stacks of the solo world's blob: 282 vertices, 560 triangles


def solo_scene(width, height):
    """The blob of scenes.mixed_test_scene alone: one MeshObject under the same transform and material, no sphere, the same sky.  The
    plain single-mesh form of the trace kernel (front_fuse 2, the normal cones, the tile entry table) runs on nothing else.  The
    tessellation is SOLO_BLOB: a triangle BVH of depth 11 (deeper than the stack minimum of 8) whose subtrees the 8 x 8 tiles of a
    64 x 40 frame can tell apart (tests/test_gpu_command_stream_solo.py says what the table holds)."""
    b = scenes.MeshSceneBuilder()
    b.add(*scenes.uv_blob(*SOLO_BLOB), scenes.trs(translate=(-2.0, 1.3, 1.0), scale=(1.2, 1.0, 0.9), yaw_deg=33.0),
          scenes._params((0.7, 0.4, 0.3), (0.2, 0.2, 0.2), (0, 0, 0), 0.6))
    mo, vv, ii, nn, bvh = b.finish()
    return scenes.Scene("solo", width, height, 4, 1, mesh_objects=mo, vertices=vv, indices=ii, normals=nn, mesh_bvh=bvh, sky=scenes.make_sky(128, 64))


def make_scene(width=64, height=40, bounces=2, world="mixed"):
    assert world in WORLDS, world
    sc = scenes.mixed_test_scene(width, height) if world == "mixed" else solo_scene(width, height)
    sc.num_bounces, sc.num_rays = bounces, 1
    return sc


def cameras(sc, world="mixed"):
    return [scenes.camera_matrices(sc.width, sc.height, position=p)[0] for p in CAMERA_POSITIONS]


def blob_span(sc):
    """(first, last) vertex of MeshObject 0 (the blob)."""
    mo = sc.mesh_objects[0]
    sl = np.asarray(sc.indices).reshape(-1)[int(mo["indices_offset"]): int(mo["indices_offset"]) + int(mo["indices_count"])]
    return int(sl.min()), int(sl.max())


def edited_scene(sc, op, world="mixed"):
    """A copy of `sc` after a scene-edit op (no array of `sc` is written).  Both sides use it: it is plain host arithmetic on the lists.
    world: the world `sc` is of (the skin, the plan and the morph targets are that world's)."""
    out = copy.copy(sc)
    if op[0] == "move_mesh":
        mo = sc.mesh_objects.copy()
        mo[op[1]]["localToWorldMatrix"] = scenes.trs(**MOVES[op[2]])
        out.mesh_objects = mo
        out.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(mo, sc.vertices, sc.indices))
    elif op[0] == "deform":
        lo, hi = blob_span(sc)
        v = np.array(sc.vertices, F).reshape(-1, 3)
        part = v[lo: hi + 1]
        centre = part.mean(axis=0, dtype=np.float64).astype(F)
        v[lo: hi + 1] = (centre + (part - centre) * F(op[1])).astype(F)
        out.vertices = v
        out.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(sc.mesh_objects, v, sc.indices))
    elif op[0] == "move_spheres":
        sp = sc.spheres.copy()
        sp["position"] = (sp["position"] + np.asarray(SHIFTS[op[1]], F)).astype(F)
        out.spheres = sp
        out.sphere_bvh = scenes.build_object_bvh(*scenes.sphere_bounds(sp))
    elif op[0] == "camera":
        out.camera_to_world = cameras(sc, world)[op[1]]
    elif op[0] in VERTEX_WRITES:
        w = pipeline_world(sc.width, sc.height, world)
        v, n = np.array(sc.vertices, F).reshape(-1, 3), np.array(sc.normals, F).reshape(-1, 3)
        if op[0] == "skin":
            import skin_ref
            _, pose, with_normals, first, count = op
            sl = slice(first, first + count)
            pos, nrm = skin_ref.skin(w["rest_v"][sl], w["rest_n"][sl] if with_normals else None, w["bone_idx"][sl], w["bone_wgt"][sl], w["poses"][pose])
            v[sl] = pos
            if with_normals:
                n[sl] = nrm
        elif op[0] == "normals":
            import normals_ref
            lo, hi = w["span"]
            n[lo: hi + 1] = normals_ref.apply(w["plan"], v)
        else:
            sl = slice(op[1], op[1] + op[2])
            part = v[sl]
            centre = part.mean(axis=0, dtype=np.float64).astype(F)
            v[sl] = (centre + (part - centre) * F(op[3])).astype(F)
        out.vertices, out.normals = v, n
        if op[0] != "normals":
            out.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(sc.mesh_objects, v, sc.indices))
    elif op[0] == "morph":
        import morph_ref
        w = dynamic_world(sc.width, sc.height, world)
        lo, hi = w["span"]
        _, j, with_normals, normalize = op
        v, n = np.array(sc.vertices, F).reshape(-1, 3), np.array(sc.normals, F).reshape(-1, 3)
        pos, nrm = morph_ref.morph(w["rest_v"], w["rest_n"] if with_normals else None, w["deltas"], lo, hi - lo + 1, MORPH_WEIGHTS[j], normalize)
        v[lo: hi + 1] = pos
        if with_normals:
            n[lo: hi + 1] = nrm
        out.vertices, out.normals = v, n
        out.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(sc.mesh_objects, v, sc.indices))
    else:
        raise ValueError(op)
    return out


def heap_kind(edit):
    """0 (meshes) | 1 (spheres): the object-level heap an op of DEVICE_EDITS makes stale."""
    return 1 if edit[0] == "move_spheres" else 0


def device_heap_of(sc, kind):
    """(leaves, heap) of kind 0 | 1 as the device builds them from the scene's lists (include/urt.h "the object-level BVH on the device":
    what urt_host_*_leaf_bounds(literal = 0) and urt_host_build_object_bvh compute, by value).  NOT scenes.mesh_bounds / sphere_bounds:
    they round outward, so their heaps differ from these by value."""
    from unityraytracer_amd import host_scene
    leaves = host_scene.sphere_leaf_bounds(sc.spheres) if kind else host_scene.mesh_leaf_bounds(sc.mesh_objects, sc.vertices, sc.indices)
    return leaves, host_scene.build_object_bvh(leaves)


def heap_words(nodes):
    """BVHNodes (28 bytes each, as bytes or as records) as (n, 7) words: the six floats as bits — +0 for a zero of either sign, the header
    promises the device's floats by value — and the index."""
    a = np.ascontiguousarray(nodes).reshape(-1).view(np.uint8).reshape(-1, 28)
    out = np.array(a.view(np.uint32).reshape(-1, 7))
    out[:, :6] = (out[:, :6].view(F) + F(0.0)).view(np.uint32)
    return out


_WORLDS = {}


def pipeline_world(width=64, height=40, world="mixed"):
    """What the pipeline profile adds to the world, from the untouched scene (made once per size): the blob's span, its rest pose in
    buffers of the vertex count, a two-bone skin with one bone table per pose, and the canonical normals plan of the span."""
    if (width, height, world) not in _WORLDS:
        import normals_ref
        import skin_ref
        sc = make_scene(width, height, world=world)
        lo, hi = blob_span(sc)
        v, n = np.array(sc.vertices, F).reshape(-1, 3), np.array(sc.normals, F).reshape(-1, 3)
        idx, wgt = np.zeros((len(v), 4), np.int32), np.zeros((len(v), 4), F)
        idx[lo: hi + 1], wgt[lo: hi + 1], _ = skin_ref.two_bone_bend(v[lo: hi + 1], 0.0)
        poses = [skin_ref.two_bone_bend(v[lo: hi + 1], a)[2] for a in POSE_ANGLES]
        rest_v, rest_n = np.zeros_like(v), np.zeros_like(n)
        rest_v[lo: hi + 1], rest_n[lo: hi + 1] = v[lo: hi + 1], n[lo: hi + 1]
        flags = np.zeros(len(sc.mesh_objects), np.int32)
        flags[0] = 1
        _WORLDS[(width, height, world)] = {"span": (lo, hi), "rest_v": rest_v, "rest_n": rest_n, "bone_idx": idx, "bone_wgt": wgt, "poses": poses,
                                    "plan": normals_ref.plan(v, sc.indices, lo, hi - lo + 1), "deformed": flags}
    return _WORLDS[(width, height, world)]


_DYNAMIC_WORLDS = {}


def dynamic_world(width=64, height=40, world="mixed"):
    """What the dynamic profile adds to pipeline_world (whose entries it holds, too), made once per size: "deltas", the urt_MorphDelta
    array of N_TARGETS sparse targets over the blob's span — served vertex i is named by target 0 when i % 2 == 0, by target 1 when
    i % 3 == 0 and by target 2 when i % 5 == 0, so some vertices are touched by none and some by all three — and "counts", the element
    counts of the four stride-28 buffers."""
    if (width, height, world) not in _DYNAMIC_WORLDS:
        import morph_ref
        w = dict(pipeline_world(width, height, world))
        sc = make_scene(width, height, world=world)
        lo, hi = w["span"]
        rng = np.random.default_rng(4242)
        vertex, target = [], []
        for t, step in enumerate((2, 3, 5)):
            at = np.arange(lo, hi + 1)[(np.arange(hi - lo + 1) % step) == 0]
            vertex.append(at)
            target.append(np.full(len(at), t))
        vertex, target = np.concatenate(vertex), np.concatenate(target)
        dp = (w["rest_n"][vertex] * F(0.35) * rng.uniform(0.5, 1.0, (len(vertex), 1)) + rng.normal(scale=0.05, size=(len(vertex), 3))).astype(F)
        dn = rng.normal(scale=0.3, size=(len(vertex), 3)).astype(F)
        w["deltas"] = morph_ref.deltas_array(vertex, target, dp, dn)
        w["counts"] = {"LM": len(sc.mesh_objects), "LS": len(sc.spheres), "HM": len(sc.mesh_bvh), "HS": len(sc.sphere_bvh)}
        _DYNAMIC_WORLDS[(width, height, world)] = w
    return _DYNAMIC_WORLDS[(width, height, world)]


def aov_targets(op):
    """The texture names an ("aov", set, mask, frame_ray) op writes, as (hit, normal, albedo, id) with None for a target not wanted."""
    names = G_TEX if op[1] == "G" else P_TEX
    return tuple(names[b] if op[2] >> b & 1 else None for b in range(4))


def query_xy(seed, width, height):
    rng = np.random.default_rng(2000 + seed)
    return np.stack([rng.integers(width, size=N_QUERIES), rng.integers(height, size=N_QUERIES)], axis=1).astype(np.int32)


def query_rays(seed):
    """64 rays from around the scene, half of them aimed into it (fixed bounds: the edits stay within them)."""
    rng = np.random.default_rng(1000 + seed)
    lo, hi = np.array([-6.0, -1.0, -6.0]), np.array([6.0, 5.0, 6.0])
    o = (lo + rng.random((N_QUERIES, 3)) * (hi - lo)).astype(F)
    d = rng.normal(size=(N_QUERIES, 3))
    aim = np.array([-2.0, 0.0, -2.0]) + rng.random((N_QUERIES, 3)) * np.array([5.0, 3.5, 4.0]) - o
    d[: N_QUERIES // 2] = aim[: N_QUERIES // 2]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(F)


def query_pixels():
    i = np.arange(N_QUERIES, dtype=np.int64)
    return np.stack([(i % 4096).astype(F), (i // 4096).astype(F)], axis=1)


# ---- programs -----------------------------------------------------------------------------------------------------------------------
class _Track:
    """What a generator / the coverage analysis has to know about the state a program has reached."""

    def __init__(self):
        self.sky, self.result, self.tickets = "S0", "T0", 0

    def other_result(self):
        return "T1" if self.result == "T0" else "T0"

    def allowed(self, op):
        k = op[0]
        if k == "frame":
            return self.sky != self.result and op[1] != "C"
        if k == "dispatch":
            return self.sky != op[1]
        if k == "history":
            return self.sky not in ("H", "N")
        if k == "blit":
            return op[1] != op[2] and size_class(op[1]) == size_class(op[2])
        if k == "read_begin":
            return self.tickets < 2
        if k == "read_end":
            return self.tickets > 0
        return True

    def apply(self, op):
        k = op[0]
        if k == "bind_sky":
            self.sky = op[1]
        elif k == "bind_result":
            self.result = self.other_result()
        elif k == "read_begin":
            self.tickets += 1
        elif k == "read_end":
            self.tickets -= 1


def writes_of(op, result):
    """[(texture, writer kind)] of an op, in order; `result` = the Result texture bound when it runs."""
    k = op[0]
    if k == "frame":
        return [(result, "frame_dispatch"), ("C", "blend")] + ([(op[1], "present")] if op[1] else [])
    if k == "dispatch":
        return [(op[1], "dispatch")]
    if k == "blit":
        return [(op[2], "blit")]
    if k == "history":
        return [("H", "history"), ("N", "history")]
    if k == "setpixels":
        return [(op[1], "setpixels")]
    return []


_WEIGHTS = {"frame": 30, "dispatch": 5, "blit": 6, "history": 5, "setpixels": 4, "restart": 2, "bind_sky": 5, "bind_result": 3, "move_mesh": 2,
            "deform": 2, "move_spheres": 2, "camera": 2, "flush": 4, "ptr": 2, "get": 5, "read_begin": 6, "read_end": 5, "ray_query": 3,
            "radiance_query": 3}


def _draw(rng, kind, tr):
    pick = lambda names: names[int(rng.integers(len(names)))]
    if kind == "frame":
        return ("frame", pick((None, "X0", "X0", "X1", "X2", "H", tr.other_result())))
    if kind == "dispatch":
        return ("dispatch", pick(("T0", "T1")))
    if kind == "blit":
        if rng.random() < 0.25:
            return ("blit", *[SKY_TEX[i] for i in rng.permutation(2)])
        a, b = rng.permutation(len(FRAME_TEX))[:2]
        return ("blit", FRAME_TEX[a], FRAME_TEX[b])
    if kind == "history":
        return ("history", float(pick((0.0, 1.0, 4.0))))
    if kind == "setpixels":
        return ("setpixels", pick(ALL_TEX), float(pick((0.0, 0.25, 1.5))))
    if kind == "bind_sky":
        return ("bind_sky", pick((None,) + ALL_TEX))
    if kind == "move_mesh":
        return ("move_mesh", int(rng.integers(2)), int(rng.integers(len(MOVES))))
    if kind == "deform":
        return ("deform", float(pick(DEFORM_SCALES)))
    if kind == "move_spheres":
        return ("move_spheres", int(rng.integers(len(SHIFTS))))
    if kind == "camera":
        return ("camera", int(rng.integers(len(CAMERA_POSITIONS))))
    if kind == "ptr":
        return ("ptr", pick(("X0", "X1", "X2", "S1", "H")))
    if kind == "get":
        return ("get", pick(ALL_TEX))
    if kind == "read_begin":
        return ("read_begin", pick(FRAME_TEX), pick(FORMATS))
    if kind in ("ray_query", "radiance_query"):
        return (kind, int(rng.integers(1 << 16)))
    return (kind,)


def make_program(seed, n_ops=40, profile="frames"):
    """About n_ops ops, deterministic per seed.  The plain draw is biased towards the cases the suite exists for: a texture that has just
    been written is bound as the sky and traced at once (every writer kind), readbacks and scene edits land between frames.
    profile="pipeline": make_pipeline_program, profile="display": make_display_program (the programs of a profile are what they were
    before the next one existed)."""
    if profile == "pipeline":
        return make_pipeline_program(seed, n_ops)
    if profile == "display":
        return make_display_program(seed, n_ops)
    if profile == "dynamic":
        return make_dynamic_program(seed, n_ops)
    if profile == "solo":
        return make_solo_program(seed, n_ops)
    assert profile == "frames", profile
    rng = np.random.default_rng(seed)
    kinds = list(_WEIGHTS)
    p = np.array([_WEIGHTS[k] for k in kinds], dtype=np.float64)
    p /= p.sum()
    tr, prog, forced = _Track(), [], []

    def emit(op):
        tr.apply(op)
        prog.append(op)

    while len(prog) < n_ops:
        if forced:
            op = forced.pop(0)
            if tr.allowed(op):
                emit(op)
            continue
        op = _draw(rng, kinds[int(rng.choice(len(kinds), p=p))], tr)
        if not tr.allowed(op):
            continue
        result = tr.result
        emit(op)
        written = [t for t, _ in writes_of(op, result) if t != tr.result]
        if op[0] == "frame":                                   # (the frame's own Result is the least interesting of what it wrote)
            written = [t for t in written if t != result] or written
        r = rng.random()
        if written and r < 0.4:                                  # written -> bound as the sky -> traced, nothing in between
            t = written[int(rng.integers(len(written)))]
            forced = [("bind_sky", t), ("frame", "X1" if t != "X1" else "X2")]
            if rng.random() < 0.5:
                forced.append(("read_begin", forced[1][1], FORMATS[int(rng.integers(3))]))
        elif op[0] in ("frame", "dispatch") and r < 0.55:        # something between two frames of what would be one batch
            mid = [("get", "C"), ("read_begin", "C", FORMATS[int(rng.integers(3))]), ("move_mesh", 0, int(rng.integers(3))), ("deform", 0.9),
                   ("move_spheres", int(rng.integers(3))), ("ray_query", 7), ("radiance_query", 7)][int(rng.integers(7))]
            forced = [mid, ("frame", None)]
    while tr.tickets:
        emit(("read_end",))
    return prog


# ---- programs of the pipeline profile ------------------------------------------------------------------------------------------------
class _PipeTrack(_Track):
    def __init__(self):
        super().__init__()
        self.camera = 0
        self.g_ready = self.p_ready = self.n_ready = False       # the guides / the previous view's buffers / the counts hold something

    def allowed(self, op):
        k = op[0]
        if k == "aov":
            return self.sky not in aov_targets(op)
        if k == "aov_into":
            return self.sky != op[1]
        if k == "reproject":
            return self.sky not in ("R", "RN", "MV")
        if k == "resample":
            return self.sky not in ("H", "N")
        if k == "denoise":
            return op[1] in EXACT_TEX                            # (sizes that differ are refused)
        if k in ("blit", "bind_sky", "read_begin", "ptr") and "D" in op[1:]:
            return False                                         # D is approximate in the model: it feeds nothing
        return super().allowed(op)

    def apply(self, op):
        super().apply(op)
        if op[0] == "camera":
            self.camera = op[1]
        elif op[0] == "aov" and op[2] & 11 == 11:
            self.g_ready, self.p_ready = self.g_ready or op[1] == "G", self.p_ready or op[1] == "P"
        elif op[0] in ("history", "resample"):
            self.n_ready = True

    def prerequisites(self, op):
        """The ops without which an image operation has nothing to work on (all-miss guides, empty counts): played in front of it."""
        pre = []
        if op[0] in ("denoise", "reproject") and not self.g_ready:
            pre.append(("aov", "G", 15, False))
        if op[0] == "reproject":
            if not self.n_ready:
                pre = [("frame", None), ("history", 0.0)] + pre
            if not self.p_ready:
                pre = [("aov", "P", 11, False)] + pre
        return pre


def pipeline_writes_of(op, result):
    """writes_of for every kind of the pipeline profile."""
    k = op[0]
    if k == "aov":
        return [(t, "aov") for t in aov_targets(op) if t]
    if k == "aov_into":
        return [(op[1], "aov")]
    if k == "reproject":
        return [("R", "reproject"), ("RN", "reproject"), ("MV", "reproject")]
    if k == "denoise":
        return [("D", "denoise")]
    if k == "resample":
        return [("H", "resample"), ("N", "resample")]
    return writes_of(op, result)


def pipeline_reads_of(op, result):
    """The textures an image operation reads (resample_below reads what it blends into)."""
    k = op[0]
    if k == "reproject":
        return [op[4], "N", "Ph", "Pn", "Pi", "Gh", "Gn", "Gi"]
    if k == "denoise":
        return [op[1], "Gh", "Gn"] + (["Ga"] if op[3] else [])
    if k == "select":
        return [op[1]]
    if k == "resample":
        return ["H", "N"]
    return []


_PIPE_WEIGHTS = {"frame": 22, "dispatch": 3, "blit": 4, "history": 6, "setpixels": 2, "restart": 1, "bind_sky": 3, "bind_result": 2, "move_mesh": 2,
                 "deform": 2, "move_spheres": 2, "camera": 3, "flush": 2, "ptr": 1, "get": 3, "read_begin": 3, "read_end": 3, "ray_query": 2,
                 "radiance_query": 3, "aov": 6, "aov_into": 4, "reproject": 5, "denoise": 4, "select": 3, "resample": 4, "radiance_pixels": 4,
                 "skin": 4, "normals": 4, "set_device": 4, "set_host": 4, "snapshot": 3, "get_buffer": 4, "bounds": 3, "ray_query_async": 4,
                 "radiance_async": 4}


def _draw_pipeline(rng, kind, tr, nv, span):
    pick = lambda names: names[int(rng.integers(len(names)))]
    lo, hi = span

    def vertex_range(within_blob):
        a, b = (lo, hi + 1) if within_blob else (0, nv)
        first = int(rng.integers(a, b - 1))
        return first, int(rng.integers(1, min(64, b - first) + 1))

    if kind == "aov":
        return ("aov", pick(("G", "P")), int(pick((15, 15, 11, 7, 4, 3))), bool(rng.random() < 0.25))
    if kind == "aov_into":
        return ("aov_into", pick((tr.result, tr.result, "C", "C", tr.other_result(), "X0", "H", "X1")))
    if kind == "reproject":
        j = tr.camera if rng.random() < 0.15 else (tr.camera + 1 + int(rng.integers(len(CAMERA_POSITIONS) - 1))) % len(CAMERA_POSITIONS)
        return ("reproject", pick(FORMS), j, float(pick((0.0, 8.0, 64.0))), pick(("C", "H")))
    if kind == "denoise":
        return ("denoise", pick(("C", "C", "H", "X0", "R", tr.result)), int(pick((1, 2, 3))), bool(rng.random() < 0.5))
    if kind == "select":
        return ("select", pick(("N", "RN", "RN")), float(pick((1.0, 2.0, 4.0))))
    if kind == "resample":
        return ("resample", float(pick((1.0, 2.0, 3.0))), int(pick((1, 2))), float(pick((0.0, 4.0))))
    if kind == "skin":
        first, count = (lo, hi - lo + 1) if rng.random() < 0.5 else vertex_range(True)
        return ("skin", int(rng.integers(len(POSE_ANGLES))), bool(rng.random() < 0.5), first, count)
    if kind in ("set_device", "set_host"):
        return (kind, *vertex_range(rng.random() < 0.7), float(pick(DEFORM_SCALES)))
    if kind == "get_buffer":
        return ("get_buffer", pick(BUFFERS), *vertex_range(False))
    if kind == "bounds":
        return ("bounds", *vertex_range(False))
    if kind in ("radiance_pixels", "ray_query_async", "radiance_async"):
        return (kind, int(rng.integers(1 << 16)))
    if kind == "blit" and rng.random() >= 0.25:
        a, b = rng.permutation(len(EXACT_TEX))[:2]
        return ("blit", EXACT_TEX[a], EXACT_TEX[b])
    if kind == "bind_sky":
        return ("bind_sky", pick((None,) + ALL_TEX + ("R", "Ga", "RN")))
    if kind == "get":
        return ("get", pick(ALL_TEX + PIPE_TEX + ("D", "R")))
    if kind == "read_begin":
        return ("read_begin", pick(EXACT_TEX), pick(FORMATS))
    return _draw(rng, kind, tr)                                  # snapshot and normals have no argument


def _pipeline_followers(rng, op, result, tr, draw, span, nv):
    """What the pipeline profile plays right behind `op` (just emitted; `result` = the Result texture bound when it ran): a list of
    ops and of callables that draw one when their turn comes.  Draws from rng exactly what make_pipeline_program always drew here."""
    lo, hi = span
    pick = lambda names: names[int(rng.integers(len(names)))]
    k, r = op[0], rng.random()
    written = [t for t, _ in pipeline_writes_of(op, result)]
    forced = []
    if k == "history" and r < 0.6:                           # the temporal step
        prev, form = tr.camera, pick(FORMS)
        other = ("camera", (prev + 1 + int(rng.integers(len(CAMERA_POSITIONS) - 1))) % len(CAMERA_POSITIONS))
        change = {"plain": other, "objects": pick((("move_mesh", 1, int(rng.integers(3))), ("move_spheres", int(rng.integers(3))))),
                  "deformed": pick((("deform", 0.9), ("skin", int(rng.integers(3)), True, lo, hi - lo + 1), ("set_device", lo, 40, 1.25)))}[form]
        forced = [("aov", "P", 11, False)] + ([("snapshot",)] if form == "deformed" else []) + [change] + \
                 ([other] if form != "plain" and rng.random() < 0.6 else []) + [("aov", "G", 15, False),
                  ("reproject", form, prev, float(pick((8.0, 64.0))), "H"), ("select", "RN", float(pick((1.0, 2.0))))]
        if rng.random() < 0.5:
            forced += [("blit", "R", "H"), ("blit", "RN", "N"), ("resample", 2.0, 1, 0.0), ("frame", "X0")]
    elif k in ("ray_query_async", "radiance_async") and r < 0.65:
        forced = [pick((("deform", 0.9), ("skin", int(rng.integers(3)), False, lo, hi - lo + 1), ("set_device", lo + 10, 50, 0.75),
                        ("move_mesh", 0, int(rng.integers(3))), ("set_host", lo, 30, 1.25)))]
        if rng.random() < 0.5:
            forced.append(("frame", None))
    elif k in ("skin", "set_device", "normals") and r < 0.45:
        forced = [("frame", pick((None, "X0")))]
    elif k in ("skin", "set_device") and r < 0.8:            # a host write over part of what the device wrote, then read back
        first = op[3] if k == "skin" else op[1]
        forced = [("set_host", first, 8, 0.9), pick((("get_buffer", "V", first, 24), ("bounds", first, 24)))]
    elif k == "set_host" and r < 0.4:                        # a run of host uploads into the mirrored buffer
        forced = [lambda: draw("set_host") for _ in range(int(rng.integers(2, 8)))] + [pick((("frame", None), ("get_buffer", "V", 0, nv)))]
    elif k == "frame" and r < 0.15:
        forced = [("aov_into", result), ("frame", None)]
    elif k in ("frame", "dispatch") and r < 0.35:            # something between two frames of what would be one batch
        forced = [pick((lambda: draw("skin"), lambda: draw("set_device"), lambda: draw("set_host"), ("normals",), ("deform", 0.9),
                        ("get", "C"), ("ray_query_async", 7), ("radiance_pixels", 7), ("aov", "G", 15, False))), ("frame", None)]
    elif written and r < 0.75:                               # written -> read by an image operation, nothing in between
        t = written[int(rng.integers(len(written)))]
        if t in ("H", "N"):
            forced = [pick((lambda: draw("select")[:1] + ("N",) + draw("select")[2:], lambda: draw("resample"),
                            lambda: draw("reproject")[:4] + ("H",)))]
        elif t in ("R", "RN", "MV"):
            forced = [pick((("select", "RN", 1.0), ("denoise", "R", 2, True), ("bind_sky", "R")))]
            if forced[0][0] == "bind_sky":
                forced.append(("frame", "X1"))
        elif t in G_TEX + P_TEX:
            forced = [pick((lambda: draw("reproject"), lambda: ("denoise", "C") + draw("denoise")[2:]))]
        elif t != "D":
            forced = [pick((lambda: ("denoise", t) + draw("denoise")[2:], lambda: draw("reproject")[:4] + (t if t in ("C", "H") else "C",),
                            ("bind_sky", t)))]
            if forced[0] == ("bind_sky", t):
                forced += [("frame", "X1" if t != "X1" else "X2")]
    return forced


def make_pipeline_program(seed, n_ops=40):
    """As make_program, over PIPE_KINDS.  The bias: an image or a buffer that has just been written meets its consumer with nothing in
    between — a written image is the input of reproject / denoise / select / resample, a device-side vertex write is followed by a frame,
    a frame's Result texture is overwritten by aov_into and traced again, an async query is followed by an in-place scene change, host
    SetData of the mirrored vertex buffer comes in runs, and the temporal step (history, feature buffers under the old and the new view,
    reproject, select) is played as a whole."""
    rng = np.random.default_rng(100000 + seed)
    w = pipeline_world()
    lo, hi = w["span"]
    nv = len(w["rest_v"])
    kinds = list(_PIPE_WEIGHTS)
    p = np.array([_PIPE_WEIGHTS[k] for k in kinds], dtype=np.float64)
    p /= p.sum()
    tr, prog, forced = _PipeTrack(), [], []

    def emit(op):
        tr.apply(op)
        prog.append(op)

    def draw(kind):
        return _draw_pipeline(rng, kind, tr, nv, (lo, hi))

    while len(prog) < n_ops or forced:
        if forced:
            op = forced.pop(0)
            if callable(op):                                     # (drawn when its turn comes: it depends on the state reached by then)
                op = op()
            if tr.allowed(op):
                emit(op)
            continue
        op = draw(kinds[int(rng.choice(len(kinds), p=p))])
        if not tr.allowed(op):
            continue
        if tr.prerequisites(op):
            forced = tr.prerequisites(op) + [op]
            continue
        result = tr.result
        emit(op)
        forced = _pipeline_followers(rng, op, result, tr, draw, (lo, hi), nv)
    while tr.tickets:
        emit(("read_end",))
    return prog


# ---- programs of the display profile -------------------------------------------------------------------------------------------------
class _DisplayTrack(_PipeTrack):
    def __init__(self):
        super().__init__()
        self.low_ready = self.ga_ready = self.ln_ready = self.framed = self.tm_ready = False

    def allowed(self, op):
        k = op[0]
        if k == "aov_low":
            return self.sky not in ("Lh", "Lm", "Lc", "Li")
        if k == "upsample":                                      # (its outputs are no input by construction: see _draw_display)
            return self.sky is None or self.sky not in op[1:3]
        if k in ("tonemap", "bloom"):
            return op[2] != self.sky and size_class(op[1]) == size_class(op[2]) and op[1] in DISPLAY_EXACT and op[2] in DISPLAY_EXACT
        if k == "meter":
            return op[1] in DISPLAY_EXACT and (not op[3] or size_class(op[1]) == 0)
        if k == "present_tm":
            return op[1] is None or (op[1] not in (self.sky, "C") and op[1] in DISPLAY_FRAME_TEX)
        if k == "get" and op[1] == "TM":
            return self.tm_ready
        if k in ("set_host", "set_device", "bounds", "get_buffer"):      # (a follower's fixed count can reach past the last vertex)
            return sum(op[-3:-1] if k in ("set_host", "set_device") else op[-2:]) <= len(pipeline_world()["rest_v"])
        return super().allowed(op)

    def apply(self, op):
        super().apply(op)
        k = op[0]
        if k == "aov_low":
            self.low_ready = True
        elif k == "aov" and op[1] == "G" and op[2] & 4:
            self.ga_ready = True
        elif k == "setpixels" and op[1] == "Ln":
            self.ln_ready = op[2] > 0
        elif k == "frame":
            self.framed = True
        elif k == "present_tm" and op[1] is None:
            self.tm_ready = True

    def prerequisites(self, op):
        pre = super().prerequisites(op)
        if op[0] == "upsample":
            if not self.g_ready or (op[4] & SKY_FROM_ALBEDO and not self.ga_ready):
                pre.append(("aov", "G", 15, False))
            if not self.low_ready:
                pre.append(("aov_low", False))
            if op[3] and not self.ln_ready:
                pre.append(("setpixels", "Ln", 1.5))
        elif op[0] == "present_tm" and not self.framed:
            pre.append(("frame", None))
        return pre


def display_writes_of(op, result):
    """pipeline_writes_of for every kind of the display profile; the exposure states (E0, E1, the master's MS) count as resources."""
    k = op[0]
    if k == "aov_low":
        return [(t, "aov") for t in ("Lh", "Lm", "Lc", "Li")]
    if k == "upsample":
        return [(op[1], "upsample")] + ([(op[2], "upsample")] if op[2] else [])
    if k in ("tonemap", "bloom"):
        return [(op[2], k)]
    if k == "meter":
        return [(STATES[op[2]], "meter")]
    if k == "state_reset":
        return [(STATES[op[1]], "state_reset")]
    if k == "present_tm":
        return [("MS", "present_tm"), (op[1] or "TM", "present_tm")]
    return pipeline_writes_of(op, result)


def display_reads_of(op, result):
    """pipeline_reads_of for every kind of the display profile (a metering reads the state it writes: its previous exposure)."""
    k = op[0]
    if k == "upsample":
        return ["Lc", "Lh", "Lm", "Li", "Gh", "Gn", "Gi"] + (["Ln"] if op[3] else []) + (["Ga"] if op[4] & SKY_FROM_ALBEDO else [])
    if k == "meter":
        return [op[1]] + (["N"] if op[3] else []) + [STATES[op[2]]]
    if k in ("tonemap", "bloom"):
        return [op[1]] + ([STATES[op[3]]] if op[3] is not None else [])
    if k == "state_get":
        return [STATES[op[1]]]
    if k == "present_tm":
        return ["C", "MS"]
    return pipeline_reads_of(op, result)


# the pipeline profile's weights at 0.6, the rare kinds and the frame loop held up; then the display kinds
_DISPLAY_WEIGHTS = dict({k: 0.6 * v for k, v in _PIPE_WEIGHTS.items()}, frame=18, dispatch=3, history=4, restart=1.5, bind_sky=3, bind_result=2,
                        ptr=1.5, read_begin=3, read_end=3,
                        aov_low=3, upsample=6, meter=8, tonemap=8, bloom=8, state_get=4, state_reset=6, master_bloom=3, present_tm=5)
_SAME_SIZE = {0: ("X0", "X1", "X2", "U", "H"), 1: SKY_TEX, 2: ("Lc", "Ln")}


def _draw_display(rng, kind, tr, nv, span):
    pick = lambda names: names[int(rng.integers(len(names)))]
    if kind == "aov_low":
        return ("aov_low", bool(rng.random() < 0.25))
    if kind == "upsample":                                       # colour and count are never an input of the call
        return ("upsample", pick(("U", "U", "X0", "H", tr.result)), pick(("UN", "N", None)), bool(rng.random() < 0.5), int(rng.integers(4)))
    if kind == "meter":
        src = pick(("C", "C", "C", "C", tr.result, "S0", "Lc") + DISPLAY_EXACT)       # any texture of any size, the id images included
        return ("meter", src, int(rng.integers(2)), bool(size_class(src) == 0 and rng.random() < 0.3), int(rng.integers(len(METER))))
    if kind in ("tonemap", "bloom"):
        src = pick(("C", "C", "C", "H", "X0", "U", tr.result, "S0", "S1", "Lc", "Lc", "R", "Ga", "Gn", "Gi", "RN", "Li", "Lm"))
        dst = src if rng.random() < 0.3 else pick(_SAME_SIZE[size_class(src)] + ((tr.result,) if size_class(src) == 0 else ()))
        state = pick((None, 0, 0, 1, 1))
        if kind == "tonemap":
            return ("tonemap", src, dst, state, pick(TONEMAP_OPS), float(pick((1.0, 1.0, 0.5, 2.0))))
        return ("bloom", src, dst, state, int(pick((1, 3, 3, 6, 16))), int(rng.random() < 0.25) * BLOOM_ONLY)
    if kind in ("state_get", "state_reset"):
        return (kind, int(rng.integers(2)))
    if kind == "master_bloom":
        return ("master_bloom", bool(rng.random() < 0.6))
    if kind == "present_tm":
        return ("present_tm", pick((None, None, "X0", "X1", "U", tr.other_result())), pick(TONEMAP_OPS))
    if kind == "setpixels":
        return ("setpixels", pick(ALL_TEX + ("Lc", "Ln", "Ln", "U")), float(pick((0.0, 0.25, 1.5))))
    if kind == "bind_sky":
        return ("bind_sky", pick((None,) + ALL_TEX + ("R", "Ga", "RN", "U", "Lc")))
    if kind == "get":
        return ("get", pick(ALL_TEX + PIPE_TEX + LOW_TEX + UP_TEX + ("TM", "TM", "D", "R")))
    if kind == "read_begin":
        return ("read_begin", pick(DISPLAY_FRAME_TEX + ("Lc", "S1")), pick(FORMATS))
    if kind == "blit" and rng.random() < 0.15:                   # within the low grid, into the colour
        return ("blit", pick(LOW_TEX[1:]), "Lc")
    return _draw_pipeline(rng, kind, tr, nv, span)


def _sky_and_frame(t):
    return [("bind_sky", t), ("frame", "X1" if t != "X1" else "X2")]


def _display_followers(rng, op, result, tr):
    """What the display profile plays right behind a display op or a frame (`op`, just emitted).  Draws from rng exactly what
    make_display_program always drew here."""
    pick = lambda names: names[int(rng.integers(len(names)))]

    def with_prerequisites(op):
        return tr.prerequisites(op) + [op]

    k, r = op[0], rng.random()
    state = int(rng.integers(2))
    if k == "frame" and r < 0.2:                             # the presented frame: meter, bloom and / or tone-map, read back
        dest = pick(("X0", "X1", "U"))
        chain = [("meter", "C", state, bool(rng.random() < 0.2), int(pick((1, 1, 3, 0))))]
        if rng.random() < 0.6:
            chain += [("bloom", "C", dest, state, int(pick((3, 6))), 0), ("tonemap", dest, dest, state, "aces", 1.0)]
        else:
            chain += [("tonemap", "C", dest, state, pick(TONEMAP_OPS), 1.0)]
        return chain + [("read_begin", dest, "RGBA8_SRGB")]
    if k == "frame" and r < 0.24:                            # in place on C or H, then a frame or the history blend
        t = pick(("C", "H"))
        return [pick((("tonemap", t, t, None, "reinhard", 1.0), ("bloom", t, t, pick((None, state)), 3, 0))),
                pick((("frame", None), ("history", 0.0)))]
    if k == "frame" and r < 0.34:                            # a display call writes the bound Result, a frame follows
        writer = pick((("tonemap", "C", tr.result, None, "aces", 1.0), ("bloom", "C", tr.result, None, 3, 0),
                       ("upsample", tr.result, None, False, WIDE_FALLBACK)))
        return with_prerequisites(writer) + [("frame", None)]
    if k == "frame" and r < 0.42:                            # the master's ToneMap, read back
        dest = pick((None, "X0", "X1"))
        return [("master_bloom", bool(rng.random() < 0.7)), ("present_tm", dest, "aces")] + \
               ([("read_begin", dest, "RGBA8_SRGB")] if dest else [("get", "TM")])
    if k == "frame" and r < 0.48:                            # upsample into the history pair, then its consumer
        return with_prerequisites(("upsample", "H", "N", bool(rng.random() < 0.5), int(rng.integers(4)))) + \
               [pick((("select", "N", 1.0), ("resample", 2.0, 1, 0.0)))]
    if k == "meter" and r < 0.5:                             # one state twice in a row below rate 1, on sources of two sizes
        a, b = pick((("C", "Lc"), ("S0", "C"), ("Lc", "S1"), ("U", "S0")))
        return [("meter", a, op[2], False, 1), ("meter", b, op[2], False, int(pick((1, 2, 3)))),
                pick((("tonemap", "C", "X0", op[2], "aces", 1.0), ("bloom", "C", "X1", op[2], 3, 0), ("state_get", op[2])))]
    if k == "bloom" and size_class(op[1]) != 1 and r < 0.6:  # bloom on a small texture, then on a larger one
        return [pick((("bloom", "S0", "S1", None, op[4], 0), ("bloom", "S1", "S1", None, 16, 0))) if size_class(op[1]) == 0 else
                pick((("bloom", "C", "X0", None, op[4], 0), ("bloom", "S0", "S1", None, op[4], 0)))]
    if k == "upsample" and (op[1] == "H" or op[2] == "N") and r < 0.6:
        return [pick((("select", "N", 1.0), ("resample", 2.0, 1, 0.0)))]
    if k in DISPLAY_WRITERS + ("present_tm",) and r < 0.8:
        dest = op[1] if k == "upsample" else op[2] if k != "present_tm" else op[1]
        if dest is not None and dest != tr.result:          # the destination is bound as the sky and traced at once
            return _sky_and_frame(dest)
    return []


def make_display_program(seed, n_ops=40):
    """As make_pipeline_program, over DISP_KINDS (what follows an op of the pipeline profile is what follows it there).  The bias of the
    display calls: a frame's blend into C is followed by its metering, a bloom or tone mapping with that state and an 8-bit readback of
    the destination, nothing waited for in between; a display call's destination is bound as the sky and traced at once; a display call
    writes the bound Result texture and a frame follows; C or H is tone-mapped or bloomed in place and a frame or the history blend
    follows; one state is metered twice in a row at a rate below 1 on sources of two sizes; bloom on a small texture is followed by
    bloom on a larger one; upsampling into H / N is followed by resample or select; ToneMap of the master follows a frame."""
    rng = np.random.default_rng(200000 + seed)
    w = pipeline_world()
    lo, hi = w["span"]
    nv = len(w["rest_v"])
    kinds = list(_DISPLAY_WEIGHTS)
    p = np.array([_DISPLAY_WEIGHTS[k] for k in kinds], dtype=np.float64)
    p /= p.sum()
    tr, prog, forced = _DisplayTrack(), [], []

    def emit(op):
        tr.apply(op)
        prog.append(op)

    def draw(kind):
        return _draw_display(rng, kind, tr, nv, (lo, hi))

    def followers(op, result):
        return _display_followers(rng, op, result, tr)

    while len(prog) < n_ops or forced:
        if forced:
            op = forced.pop(0)
            if callable(op):
                op = op()
            drawn = op[0] == "drawn"                             # the drawn op behind its prerequisites: it has its followers, too
            op = op[1] if drawn else op
            if not tr.allowed(op):
                continue
        else:
            op, drawn = draw(kinds[int(rng.choice(len(kinds), p=p))]), True
            if not tr.allowed(op):
                continue
            if tr.prerequisites(op):
                forced = tr.prerequisites(op) + [("drawn", op)]
                continue
        result = tr.result
        emit(op)
        if not drawn:
            continue
        if op[0] in DISPLAY_KINDS or (op[0] == "frame" and rng.random() < 0.6):
            forced = followers(op, result)
        else:
            forced = _pipeline_followers(rng, op, result, tr, draw, (lo, hi), nv)
    while tr.tickets:
        emit(("read_end",))
    return prog


# ---- programs of the dynamic profile -------------------------------------------------------------------------------------------------
class _DynamicTrack(_DisplayTrack):
    def __init__(self):
        super().__init__()
        self.master_dof = None                                   # the preset EnableDepthOfField was last given (None: off)

    def allowed(self, op):
        k = op[0]
        if k == "morph":                                         # (URT_MORPH_NORMALIZE without dst_normals is refused)
            return 0 <= op[1] < len(MORPH_WEIGHTS) and (op[2] or not op[3])
        if k == "device_heap":
            return op[1][0] in DEVICE_EDITS and self.allowed(op[1])
        if k == "rebuild_heap":
            return op[1] in (0, 1)
        if k == "dof":                                           # sizes that differ; a destination that is an input or the bound sky
            _, src, hit, dst, j = op
            cls = 2 if hit == "Lh" else 0
            return hit in ("Gh", "Ph", "Lh") and src in DISPLAY_EXACT and dst in DISPLAY_EXACT and 0 <= j < len(DOF) and \
                size_class(src) == size_class(dst) == cls and dst not in (src, hit, self.sky)
        if k == "master_dof":
            return op[1] is None or 0 <= op[1] < len(DOF)
        if k == "get_buffer" and op[1] in HEAP_BUFFERS:
            return 0 <= op[2] and op[3] >= 1 and op[2] + op[3] <= dynamic_world()["counts"][op[1]]
        return super().allowed(op)

    def apply(self, op):
        super().apply(op)
        if op[0] == "master_dof":
            self.master_dof = op[1]
        elif op[0] == "device_heap":
            super().apply(op[1])

    def prerequisites(self, op):
        pre = super().prerequisites(op)
        if op[0] == "dof":                                       # a hit image nothing has rendered makes every pixel pass through
            ready = {"Gh": self.g_ready, "Ph": self.p_ready, "Lh": self.low_ready}[op[2]]
            if not ready:
                pre.append({"Gh": ("aov", "G", 15, False), "Ph": ("aov", "P", 11, False), "Lh": ("aov_low", False)}[op[2]])
        return pre


def dynamic_writes_of(op, result):
    """display_writes_of for every kind of the dynamic profile (textures and states; the buffers are dynamic_coverage's own business)."""
    if op[0] == "dof":
        return [(op[3], "dof")]
    if op[0] == "device_heap":
        return []
    return display_writes_of(op, result)


def dynamic_reads_of(op, result):
    if op[0] == "dof":
        return [op[1], op[2]]
    return display_reads_of(op, result)


# the display profile's weights at 0.75, the frame loop held up; then the dynamic kinds
_DYNAMIC_WEIGHTS = dict({k: 0.75 * v for k, v in _DISPLAY_WEIGHTS.items()}, frame=18, get_buffer=4, ray_query_async=3, present_tm=4,
                        morph=6, device_heap=9, rebuild_heap=3, dof=8, master_dof=3)
_DOF_DST = {0: ("X0", "X1", "X2", "U", "H"), 2: ("Lc", "Ln")}


def _draw_dynamic(rng, kind, tr, nv, span):
    pick = lambda names: names[int(rng.integers(len(names)))]
    lo, hi = span
    if kind == "morph":
        with_normals = bool(rng.random() < 0.6)
        return ("morph", int(rng.integers(len(MORPH_WEIGHTS))), with_normals, bool(with_normals and rng.random() < 0.5))
    if kind == "device_heap":
        edit = pick(("move_mesh", "move_mesh", "deform", "move_spheres", "move_spheres", "skin", "set_device", "set_host", "set_host", "morph"))
        return ("device_heap", _draw_dynamic(rng, edit, tr, nv, span))
    if kind == "rebuild_heap":
        return ("rebuild_heap", int(rng.integers(2)))
    if kind == "dof":
        low = rng.random() < 0.3
        hit = "Lh" if low else pick(("Gh", "Gh", "Ph"))
        src = "Lc" if low else pick(("C", "C", "C", "H", "X0", "U", tr.result, "R", "Ga"))
        dst = pick(tuple(t for t in _DOF_DST[2 if low else 0] + (() if low else (tr.result, tr.result)) if t != src))
        return ("dof", src, hit, dst, int(rng.integers(len(DOF))))
    if kind == "master_dof":
        return ("master_dof", int(rng.integers(len(DOF))) if rng.random() < 0.7 else None)
    if kind == "get_buffer" and rng.random() < 0.5:
        which = pick(HEAP_BUFFERS)
        n = dynamic_world()["counts"][which]
        first = int(rng.integers(n))
        return ("get_buffer", which, first, int(rng.integers(1, n - first + 1)))
    return _draw_display(rng, kind, tr, nv, span)


def _dynamic_followers(rng, op, result, tr, draw):
    """What the dynamic profile plays right behind a dynamic op, an async query or (for some of them) a frame."""
    pick = lambda names: names[int(rng.integers(len(names)))]
    k, r = op[0], rng.random()

    def device_heap(*kinds):
        return lambda: ("device_heap", draw(pick(kinds)))

    if k == "frame" and r < 0.3:                                 # a device build inside what would be one batch, an earlier present read back
        build = pick((device_heap("move_mesh", "move_spheres"), device_heap("set_host", "deform"), device_heap("morph", "skin"),
                      lambda: draw("rebuild_heap")))
        return [("frame", "X0"), build, ("frame", None)] + ([("read_begin", "X0", pick(FORMATS))] if rng.random() < 0.5 else [])
    if k == "frame" and r < 0.5:                                 # depth of field of what the deferred frame wrote
        if rng.random() < 0.4:
            return tr.prerequisites(("dof", "C", "Gh", tr.result, 0)) + [("dof", "C", "Gh", tr.result, int(rng.integers(len(DOF)))), ("frame", None)]
        dst = pick(("X0", "X1", "U"))
        return [("aov", "G", 15, False), ("frame", None), ("dof", pick(("C", tr.result)), "Gh", dst, int(rng.integers(len(DOF))))]
    if k == "frame" and r < 0.62:                                # the master's ToneMap with depth of field on, then the next frame
        dest = pick((None, "X0", "X1"))
        return [("master_dof", int(rng.integers(len(DOF)))), ("master_bloom", bool(rng.random() < 0.5)), ("present_tm", dest, pick(TONEMAP_OPS)),
                ("frame", None)] + ([("get", "TM")] if dest is None else [("read_begin", dest, "RGBA8_SRGB")])
    if k in ("ray_query_async", "radiance_async") and r < 0.7:   # the query is left waiting across a device build
        return [pick((device_heap("deform", "set_host"), device_heap("move_mesh"), device_heap("morph", "skin")))] + \
               ([("frame", None)] if rng.random() < 0.5 else [])
    if k == "morph" and r < 0.45:                                # the host rewrites W while the first kernel may still wait for its turn
        j = (op[1] + 1 + int(rng.integers(len(MORPH_WEIGHTS) - 1))) % len(MORPH_WEIGHTS)
        return [("morph", j, op[2], op[3])] + ([("frame", None)] if rng.random() < 0.6 else [("get_buffer", "V", 0, 64)])
    if k == "morph" and r < 0.75:
        return [pick((("rebuild_heap", 0), ("frame", None), ("get_buffer", "V", 0, 64)))]
    if k in ("skin", "set_host", "deform") and r < 0.4:
        return [("rebuild_heap", 0)] + ([("frame", None)] if rng.random() < 0.6 else [])
    if k in ("device_heap", "rebuild_heap"):
        kind = heap_kind(op[1]) if k == "device_heap" else op[1]
        heap, leaves = ("HS", "LS") if kind else ("HM", "LM")
        n = dynamic_world()["counts"]
        if r < 0.35:
            return [("frame", pick((None, "X0")))]
        if r < 0.6:                                              # the SyncObjectHeaps download
            return [pick((("get_buffer", heap, 0, n[heap]), ("get_buffer", heap, 1, 2), ("get_buffer", leaves, 0, n[leaves]))), ("frame", None)]
        if r < 0.85:                                             # the host writes the heap that the device has just written
            return [(lambda: draw("move_spheres")) if kind else pick((lambda: draw("move_mesh"), lambda: draw("set_host"), lambda: draw("morph")))] + \
                   ([("frame", None)] if rng.random() < 0.7 else [])
        return []
    if k == "dof":
        if size_class(op[3]) == 2 and r < 0.6:                   # the scratch grows: a frame-sized call behind one on the low grid
            return tr.prerequisites(("dof", "C", "Gh", "X0", 0)) + [("frame", None), ("dof", "C", "Gh", pick(("X0", "X1")), int(rng.integers(len(DOF))))]
        if op[3] != tr.result and r < 0.7:                       # the destination is bound as the sky and traced at once
            return _sky_and_frame(op[3])
        if op[3] == tr.result and r < 0.8:
            return [("frame", None)]
    return []


def make_dynamic_program(seed, n_ops=40):
    """As make_display_program, over DYN_KINDS (what follows an op of the older profiles is mostly what follows it there).  The bias of
    the dynamic ops: a device build of a heap sits between two frames of what would be one batch, behind a host upload of vertices, a
    morph or a skin, with an async query left waiting across it; the heap it wrote is read back or overwritten by the host at once; a
    morph follows a morph under another weight table; depth of field reads what a deferred frame wrote, writes the bound Result or
    the next sky, and a frame-sized call follows one on the low grid; the master's ToneMap with depth of field on is followed by a frame."""
    rng = np.random.default_rng(300000 + seed)
    w = dynamic_world()
    lo, hi = w["span"]
    nv = len(w["rest_v"])
    kinds = list(_DYNAMIC_WEIGHTS)
    p = np.array([_DYNAMIC_WEIGHTS[k] for k in kinds], dtype=np.float64)
    p /= p.sum()
    tr, prog, forced = _DynamicTrack(), [], []

    def emit(op):
        tr.apply(op)
        prog.append(op)

    def draw(kind):
        return _draw_dynamic(rng, kind, tr, nv, (lo, hi))

    while len(prog) < n_ops or forced:
        if forced:
            op = forced.pop(0)
            if callable(op):
                op = op()
            drawn = op[0] == "drawn"
            op = op[1] if drawn else op
            if not tr.allowed(op):
                continue
        else:
            op, drawn = draw(kinds[int(rng.choice(len(kinds), p=p))]), True
            if not tr.allowed(op):
                continue
            if tr.prerequisites(op):
                forced = tr.prerequisites(op) + [("drawn", op)]
                continue
        result = tr.result
        emit(op)
        if not drawn:
            continue
        k = op[0]
        if k in DYNAMIC_KINDS or (k in ("frame", "ray_query_async", "radiance_async", "morph", "skin", "set_host", "deform") and rng.random() < 0.5):
            forced = _dynamic_followers(rng, op, result, tr, draw)
        elif k in DISPLAY_KINDS or (k == "frame" and rng.random() < 0.6):
            forced = _display_followers(rng, op, result, tr)
        else:
            forced = _pipeline_followers(rng, op, result, tr, draw, (lo, hi), nv)
    while tr.tickets:
        emit(("read_end",))
    return prog


# ---- programs of the solo profile ----------------------------------------------------------------------------------------------------
# The solo world (make_scene(world="solo")): one MeshObject, no sphere.  The profile's ops are the dynamic profile's that mean something
# without spheres — no move_spheres, no device_heap of it, no rebuild_heap 1, no get_buffer of HS / LS (zero-count buffers do not exist);
# move_mesh always moves object 0 — and
#     ("motion_blur", src, hit, dst, j)   ctx.motion_blur(src, MV, hit, dst, **MBLUR[j]): hit is Gh | Ph, src any exact frame-sized texture,
#                                         dst any frame-sized texture but src, MV, hit and the bound sky (the library refuses those)
MBLUR_FLAG_VELOCITY = 1                                          # URT_MOTION_BLUR_FLAG_VELOCITY
MBLUR = (dict(), dict(shutter=1.0, max_radius=4.0), dict(shutter=0.25, max_radius=0.5), dict(flags=MBLUR_FLAG_VELOCITY))
SOLO_KINDS = tuple(k for k in DYN_KINDS if k != "move_spheres") + ("motion_blur",)
SOLO_IMAGE_OPS = DYNAMIC_IMAGE_OPS + ("motion_blur",)
SOLO_WRITERS = DISPLAY_WRITERS + ("motion_blur",)
SOLO_VERTEX_WRITES = ("skin", "morph", "set_device", "set_host")


def solo_fix(op):
    """An op a follower of the older profiles plays, as the solo world means it: the spheres' ops become the mesh's, every move_mesh moves
    object 0, the sphere heap's readbacks become the mesh heap's (one leaf, one node)."""
    k = op[0]
    if k == "move_spheres":
        return ("move_mesh", 0, op[1] % len(MOVES))
    if k == "move_mesh":
        return ("move_mesh", 0, op[2])
    if k == "device_heap":
        return ("device_heap", solo_fix(op[1]))
    if k == "rebuild_heap":
        return ("rebuild_heap", 0)
    if k == "get_buffer" and op[1] in HEAP_BUFFERS:
        return ("get_buffer", {"HS": "HM", "LS": "LM"}.get(op[1], op[1]), 0, 1)
    return op


class _SoloTrack(_DynamicTrack):
    def __init__(self):
        super().__init__()
        self.mv_ready = False                                    # a reproject has written MV
        self.nv = len(pipeline_world(world="solo")["rest_v"])

    def allowed(self, op):
        k = op[0]
        if k == "move_spheres" or "HS" in op[1:] or "LS" in op[1:]:
            return False
        if k == "move_mesh":
            return op[1] == 0 and 0 <= op[2] < len(MOVES)
        if k == "rebuild_heap":
            return op[1] == 0
        if k == "get_buffer" and op[1] in ("HM", "LM"):
            return op[2:] == (0, 1)
        if k in ("set_host", "set_device", "bounds", "get_buffer"):
            first, count = op[-3:-1] if k in ("set_host", "set_device") else op[-2:]
            return 0 <= first and count >= 1 and first + count <= self.nv
        if k == "motion_blur":                                   # sizes that differ; a destination that is an input or the bound sky
            _, src, hit, dst, j = op
            if not (hit in ("Gh", "Ph") and self.mv_ready and (self.g_ready if hit == "Gh" else self.p_ready)):
                return False                                     # (a prerequisite that was refused: nothing to blur along)
            return src in DISPLAY_FRAME_TEX and dst in DISPLAY_FRAME_TEX and 0 <= j < len(MBLUR) and dst not in (src, "MV", hit, self.sky)
        return super().allowed(op)

    def apply(self, op):
        super().apply(op)
        if op[0] == "reproject":
            self.mv_ready = True

    def prerequisites(self, op):
        pre = super().prerequisites(op)
        if op[0] == "motion_blur":                               # a motion image nothing has written makes every tile still
            if not self.mv_ready:
                rp = ("reproject", "plain", (self.camera + 1) % len(CAMERA_POSITIONS), 8.0, "C")
                pre += super().prerequisites(rp) + [rp]
            want = ("aov", "G", 15, False) if op[2] == "Gh" else ("aov", "P", 11, False)
            if not (self.g_ready if op[2] == "Gh" else self.p_ready) and want not in pre:      # (the reproject's own may render both sets)
                pre.append(want)
        return pre


def solo_writes_of(op, result):
    if op[0] == "motion_blur":
        return [(op[3], "motion_blur")]
    return dynamic_writes_of(op, result)


def solo_reads_of(op, result):
    if op[0] == "motion_blur":
        return [op[1], "MV", op[2]]
    return dynamic_reads_of(op, result)


# the dynamic profile's weights without the spheres' kind, the frame loop and the vertex writes held up; then motion blur
_SOLO_WEIGHTS = dict({k: v for k, v in _DYNAMIC_WEIGHTS.items() if k != "move_spheres"}, frame=20, camera=3, bind_result=2.5, skin=4, set_device=3,
                     set_host=3, morph=5, device_heap=6, dof=4, motion_blur=9)


def _draw_solo(rng, kind, tr, nv, span):
    pick = lambda names: names[int(rng.integers(len(names)))]
    if kind == "motion_blur":
        src = pick(("C", "C", "C", "H", "X0", "U", tr.result, "R"))
        dst = pick(tuple(t for t in ("X0", "X1", "X2", "U", "H", tr.result, tr.result) if t != src))
        return ("motion_blur", src, pick(("Gh", "Gh", "Ph")), dst, int(rng.integers(len(MBLUR))))
    if kind == "move_mesh":
        return ("move_mesh", 0, int(rng.integers(len(MOVES))))
    if kind == "device_heap":
        edit = pick(("move_mesh", "move_mesh", "deform", "skin", "set_device", "set_host", "set_host", "morph"))
        return ("device_heap", _draw_solo(rng, edit, tr, nv, span))
    if kind == "rebuild_heap":
        return ("rebuild_heap", 0)
    if kind == "get_buffer" and rng.random() < 0.3:
        return ("get_buffer", pick(("HM", "LM")), 0, 1)
    if kind == "get_buffer":
        return _draw_pipeline(rng, kind, tr, nv, span)
    return solo_fix(_draw_dynamic(rng, kind, tr, nv, span))


def _solo_followers(rng, op, result, tr, draw):
    """What the solo profile plays right behind a motion blur, a vertex write or (for some of them) a frame."""
    pick = lambda names: names[int(rng.integers(len(names)))]
    k, r = op[0], rng.random()
    if k == "frame" and r < 0.12:                                # a camera change inside what would be one batch
        return [("camera", (tr.camera + 1 + int(rng.integers(len(CAMERA_POSITIONS) - 1))) % len(CAMERA_POSITIONS)), ("frame", pick((None, "X0")))]
    if k == "frame" and r < 0.3:                                 # ... or a scene edit
        mid = pick((("deform", float(pick((1.25, 0.75)))), lambda: draw("skin"), lambda: draw("skin"), lambda: draw("morph"),
                    lambda: draw("set_device"), lambda: draw("set_host"), lambda: draw("device_heap"), lambda: draw("move_mesh")))
        return [mid, ("frame", pick((None, "X0")))]
    if k == "frame" and r < 0.42:                                # the other Result texture under the same camera
        return [("bind_result",), ("frame", None)]
    if k == "frame" and r < 0.75:                                # motion blur of what a deferred frame wrote
        hit, j = pick(("Gh", "Gh", "Ph")), int(rng.integers(len(MBLUR)))
        dst = pick((tr.result, "X1", "X0", "U"))
        blur = ("motion_blur", pick(("C", "C", tr.result if dst != tr.result else "C")), hit, dst, j)
        tail = [("frame", None)] if dst == tr.result else _sky_and_frame(dst) if rng.random() < 0.6 else []
        return tr.prerequisites(blur) + [("frame", None), blur] + tail
    if k == "motion_blur":
        if r < 0.35:                                             # the same once more under another preset
            return [op[:4] + ((op[4] + 1 + int(rng.integers(len(MBLUR) - 1))) % len(MBLUR),)]
        if op[3] != tr.result and r < 0.7:                       # the destination is bound as the sky and traced at once
            return _sky_and_frame(op[3])
        if op[3] == tr.result and r < 0.8:
            return [("frame", None)]
    if k in SOLO_VERTEX_WRITES and r < 0.7:                      # the frame's preparation reads what nothing has waited for
        return [("frame", pick((None, "X0")))]
    return []


def make_solo_program(seed, n_ops=40):
    """As make_dynamic_program, over SOLO_KINDS in the solo world, with a random stream, weights, a tracker and followers of its own (what
    follows an op of the older profiles is mostly what follows it there, through solo_fix).  The bias of this profile: a camera change or a
    scene edit sits between two frames of what would be one batch (the tile entry table of the launch behind it is another one), the
    Result texture is swapped between two frames of one camera (the same table), a vertex write of every kind is followed by a frame
    with nothing that looks at the vertices in between, motion blur reads what a deferred frame wrote, writes the bound Result or the
    next sky, and is called twice under two presets."""
    rng = np.random.default_rng(400000 + seed)
    w = dynamic_world(world="solo")
    lo, hi = w["span"]
    nv = len(w["rest_v"])
    kinds = list(_SOLO_WEIGHTS)
    p = np.array([_SOLO_WEIGHTS[k] for k in kinds], dtype=np.float64)
    p /= p.sum()
    tr, prog, forced = _SoloTrack(), [], []

    def emit(op):
        tr.apply(op)
        prog.append(op)

    def draw(kind):
        return _draw_solo(rng, kind, tr, nv, (lo, hi))

    while len(prog) < n_ops or forced:
        if forced:
            op = forced.pop(0)
            if callable(op):
                op = op()
            drawn = op[0] == "drawn"
            op = solo_fix(op[1] if drawn else op)
            if not tr.allowed(op):
                continue
        else:
            op, drawn = draw(kinds[int(rng.choice(len(kinds), p=p))]), True
            if not tr.allowed(op):
                continue
            if tr.prerequisites(op):
                forced = tr.prerequisites(op) + [("drawn", op)]
                continue
        result = tr.result
        emit(op)
        if not drawn:
            continue
        k = op[0]
        if k == "motion_blur" or (k in ("frame",) + SOLO_VERTEX_WRITES and rng.random() < 0.6):
            forced = _solo_followers(rng, op, result, tr, draw)
        elif k in DYNAMIC_KINDS or (k in ("frame", "ray_query_async", "radiance_async", "morph", "skin", "set_host", "deform") and rng.random() < 0.5):
            forced = _dynamic_followers(rng, op, result, tr, draw)
        elif k in DISPLAY_KINDS or (k == "frame" and rng.random() < 0.6):
            forced = _display_followers(rng, op, result, tr)
        else:
            forced = _pipeline_followers(rng, op, result, tr, draw, (lo, hi), nv)
    while tr.tickets:
        emit(("read_end",))
    return prog


# the ops that leave the deferred frames deferred (dynamic_coverage's "quiet" ops); every other op has submitted them when it returns
SOLO_QUIET = ("restart", "bind_sky", "bind_result", "camera", "master_bloom", "master_dof", "frame", "dispatch", "snapshot", "ray_query_async",
              "radiance_async", "morph", "device_heap", "rebuild_heap") + SCENE_CHANGES


SOLO_CASES = ("edit_between_frames", "camera_between_frames", "bind_result_between_frames", "blur_input_deferred", "blur_into_result_or_sky",
              "write_then_frame_skin", "write_then_frame_morph", "write_then_frame_set_device", "write_then_frame_set_host", "two_presets")


def solo_coverage(program):
    """Static facts about a program of the solo profile (tests/test_command_stream_model.py holds the seed set to them).  "Quiet" ops are
    dynamic_coverage's: they leave the deferred frames deferred.  A frame is OPEN while it could still be deferred: nothing but quiet ops
    has run since.
    kinds: op kind -> count (a wrapped edit counts as device_heap);
    edit_between_frames / camera_between_frames: scene changes (device builds and morphs included) / camera ops with an open frame in
    front of them and a frame behind them before anything that is not quiet — and, for a scene change, no camera op between those two
    frames: both are the same camera's, only the scene differs;
    bind_result_between_frames: bind_result ops likewise, no camera op between the two frames;
    blur_input_deferred: motion_blur ops whose source or hit image was written by an open frame;
    blur_into_result_or_sky: motion_blur ops that write the bound Result texture with a frame after them, or whose destination is bound
    as the sky after the write and traced before anything else writes it;
    write_then_frame_K, K of skin | morph | set_device | set_host: vertex writes of that kind (wrapped ones included) with a frame behind
    them and nothing between that reads V or prepares the scene;
    two_presets: 1 when the program's motion_blur ops use two presets or more."""
    kinds = {k: 0 for k in SOLO_KINDS}
    tr = _SoloTrack()
    quiet = SOLO_QUIET
    readers_of_v = ("get_buffer", "bounds", "snapshot", "aov", "aov_into", "aov_low", "ray_query", "radiance_query", "radiance_pixels", "resample",
                    "ray_query_async", "radiance_async", "present_tm", "dispatch", "normals", "rebuild_heap", "reproject")
    out = {key: 0 for key in SOLO_CASES}
    deferred, pending, presets = set(), 0, set()
    last_writer, write_at, bound_at, counted = {}, {}, -1, set()
    frames_after = np.cumsum([op[0] in ("frame", "dispatch") for op in program][::-1])[::-1]

    def frame_behind(i, no_camera):
        """A frame follows op i before anything that is not quiet (and before a camera op, if no_camera)."""
        for q in program[i + 1:]:
            if q[0] == "frame":
                return True
            if q[0] not in quiet or (no_camera and q[0] == "camera"):
                return False
        return False

    def camera_since_frame(i):
        for q in program[:i][::-1]:
            if q[0] in ("frame", "dispatch"):
                return False
            if q[0] == "camera":
                return True
        return False

    for i, op in enumerate(program):
        k = op[0]
        kinds[k] += 1
        result = tr.result if k != "dispatch" else op[1]
        edit = op[1] if k == "device_heap" else op if k in DEVICE_EDITS else None
        if edit is not None:
            out["edit_between_frames"] += bool(pending > 0 and not camera_since_frame(i) and frame_behind(i, True))
            if edit[0] in SOLO_VERTEX_WRITES:
                behind = None
                for q in program[i + 1:]:
                    if q[0] == "frame" or q[0] in readers_of_v or (q[0] == "device_heap"):
                        behind = q[0]
                        break
                out["write_then_frame_" + edit[0]] += behind == "frame"
        if k == "camera":
            out["camera_between_frames"] += bool(pending > 0 and frame_behind(i, False))
        if k == "bind_result":
            out["bind_result_between_frames"] += bool(pending > 0 and not camera_since_frame(i) and frame_behind(i, True))
        if k == "motion_blur":
            presets.add(op[4])
            out["blur_input_deferred"] += bool(deferred & {op[1], op[2]})
            out["blur_into_result_or_sky"] += bool(op[3] == tr.result and frames_after[i] > 0)
        if k in ("frame", "dispatch") and tr.sky in last_writer and bound_at > write_at[tr.sky] and (tr.sky, write_at[tr.sky]) not in counted:
            counted.add((tr.sky, write_at[tr.sky]))
            out["blur_into_result_or_sky"] += last_writer[tr.sky] == "motion_blur"
        # the state after the op
        if k in ("frame", "dispatch"):
            pending += 1
            deferred |= {t for t, _ in writes_of(op, result)}
        elif k not in quiet:
            pending, deferred = 0, set()
        for t, wk in solo_writes_of(op, result):
            last_writer[t], write_at[t] = wk, i
        if k == "bind_sky":
            bound_at = i
        tr.apply(op)
    out["two_presets"] = int(len(presets) >= 2)
    out["kinds"] = kinds
    return out


def dynamic_coverage(program):
    """Static facts about a program of the dynamic profile (tests/test_command_stream_model.py holds the seed set to them).  A DEVICE BUILD
    is a device_heap or a rebuild_heap op; "quiet" ops are the ones of display_coverage and the dynamic ones but dof (a device build
    and a morph enqueue on the context's stream and leave the deferred frames deferred).  A heap is DEVICE-WRITTEN from its device
    build until something takes it: the next op that prepares the scene, a get_buffer of it, or a host SetData of it.
    kinds: op kind -> count (a wrapped edit counts as device_heap);
    build_between_frames: device builds with a deferred frame in front of them and a frame directly behind;
    build_behind_upload / build_behind_morph_or_skin: device builds whose vertices were last written by deform / set_host, or by morph /
    skin, since the scene was last prepared (the wrapped edit included);
    host_write_of_device_heap: host SetData of a heap (an unwrapped edit of its kind) while it is device-written;
    get_device_heap: get_buffer of HM / HS while it is device-written;
    morph_after_morph: a morph directly behind a morph with another weight table;
    async_across_build: device builds reached while an async query has not been observed;
    dof_input_deferred: dof ops whose source or hit was written by frames that could still be deferred;
    dof_into_result: dof ops that write the bound Result texture, with a frame after them;
    dof_regrow: frame-sized dof ops behind a dof on the low grid and before any other frame-sized one;
    master_dof_then_frame: present_tm with depth of field on whose next op that is not a binding is a frame;
    dof_sky_traced: dof destinations bound as the sky after the write and traced before anything else wrote them."""
    kinds = {k: 0 for k in DYN_KINDS}
    tr = _DynamicTrack()
    neutral = ("restart", "bind_sky", "bind_result", "camera", "master_bloom", "master_dof")
    quiet = neutral + ("frame", "dispatch", "snapshot", "ray_query_async", "radiance_async", "morph", "device_heap", "rebuild_heap") + SCENE_CHANGES
    prepares = ("frame", "dispatch", "aov", "aov_into", "aov_low", "ray_query", "radiance_query", "radiance_pixels", "resample", "ray_query_async",
                "radiance_async", "present_tm")
    out = {key: 0 for key in ("build_between_frames", "build_behind_upload", "build_behind_morph_or_skin", "host_write_of_device_heap",
                              "get_device_heap", "morph_after_morph", "async_across_build", "dof_input_deferred", "dof_into_result", "dof_regrow",
                              "master_dof_then_frame", "dof_sky_traced")}
    deferred, pending, async_open, vertex_writer, device_written = set(), 0, False, None, [False, False]
    last_writer, write_at, bound_at, counted, low_dof_open = {}, {}, -1, set(), False
    frames_after = np.cumsum([op[0] in ("frame", "dispatch") for op in program][::-1])[::-1]
    for i, op in enumerate(program):
        k = op[0]
        kinds[k] += 1
        result = tr.result if k != "dispatch" else op[1]
        edit = op[1] if k == "device_heap" else op if k in DEVICE_EDITS else None
        following = [q[0] for q in program[i + 1:] if q[0] not in neutral][:1]
        if edit is not None and edit[0] in ("deform", "set_host"):
            vertex_writer = "upload"
        elif edit is not None and edit[0] in ("morph", "skin"):
            vertex_writer = "device"
        if k in ("device_heap", "rebuild_heap"):
            kind = heap_kind(op[1]) if k == "device_heap" else op[1]
            out["build_between_frames"] += bool(pending > 0 and program[i + 1: i + 2] and program[i + 1][0] == "frame")
            out["build_behind_upload"] += bool(kind == 0 and vertex_writer == "upload")
            out["build_behind_morph_or_skin"] += bool(kind == 0 and vertex_writer == "device")
            out["async_across_build"] += bool(async_open)
            device_written[kind] = True
        elif edit is not None:                                   # an unwrapped edit: the host writes the heap of its kind
            out["host_write_of_device_heap"] += bool(device_written[heap_kind(edit)])
            device_written[heap_kind(edit)] = False
        if k == "get_buffer" and op[1] in ("HM", "HS"):
            out["get_device_heap"] += bool(device_written[op[1] == "HS"])
            device_written[op[1] == "HS"] = False
        if k == "morph":
            before = program[i - 1] if i else ("",)
            out["morph_after_morph"] += bool(before[0] == "morph" and MORPH_WEIGHTS[before[1]] != MORPH_WEIGHTS[op[1]])
        if k == "dof":
            frame_sized = size_class(op[3]) == 0
            out["dof_input_deferred"] += bool(deferred & set(dynamic_reads_of(op, result)))
            out["dof_into_result"] += bool(op[3] == tr.result and frames_after[i] > 0)
            out["dof_regrow"] += bool(frame_sized and low_dof_open)
            low_dof_open = not frame_sized
        if k == "present_tm":
            out["master_dof_then_frame"] += bool(tr.master_dof is not None and following == ["frame"])
        if k in ("frame", "dispatch") and tr.sky in last_writer and bound_at > write_at[tr.sky] and (tr.sky, write_at[tr.sky]) not in counted:
            counted.add((tr.sky, write_at[tr.sky]))
            out["dof_sky_traced"] += last_writer[tr.sky] == "dof"
        # the state after the op
        if k in OBSERVERS:
            async_open = False
        if k in ("ray_query_async", "radiance_async"):
            async_open = True
        if k in prepares:
            vertex_writer, device_written = None, [False, False]
        if k in ("frame", "dispatch"):
            pending += 1
            deferred |= {t for t, _ in writes_of(op, result)}
        elif k not in quiet:
            pending, deferred = 0, set()
        for t, wk in dynamic_writes_of(op, result):
            last_writer[t], write_at[t] = wk, i
        if k == "bind_sky":
            bound_at = i
        tr.apply(op)
    out["kinds"] = kinds
    return out


def display_coverage(program):
    """Static facts about a program of the display profile (tests/test_command_stream_model.py holds the seed set to them).  "Quiet" ops
    are the ones that neither submit the deferred frames nor wait: frames and dispatches themselves, scene and vertex edits, bindings.
    kinds: op kind -> count;
    input_deferred: display image calls (upsample, meter, tonemap, bloom, present_tm) that read a texture frames wrote while those frames
    could still be deferred;  output_deferred: such calls that write one, with a frame after them;
    state_chain: bloom / tonemap calls reading a state whose last metering read such a texture, with nothing but quiet ops and other
    bloom / tonemap calls since that metering (nothing has waited: the state is read on the device behind its writer);
    in_place_then_frame: tonemap / bloom with dst = src whose next op that is not a binding is a frame, a dispatch or the history blend;
    written_then_sky_traced: writer kind -> textures last written by it that were bound as the sky after that write and traced before
    anything else wrote them;
    writes_bound_result: display image calls that write the bound Result texture, with a frame after them;
    pyramid_regrow: bloom calls that need more pyramid texels than every bloom before them in the program (there is one before);
    two_meterings_rate_below_1: a metering at a rate below 1 right behind another one of the same state, on a source of another size."""
    kinds = {k: 0 for k in DISP_KINDS}
    tr = _DisplayTrack()
    neutral = ("restart", "bind_sky", "bind_result", "camera", "master_bloom")
    quiet = neutral + ("frame", "dispatch", "snapshot", "ray_query_async", "radiance_async") + SCENE_CHANGES
    sizes = {0: (64, 40), 1: make_scene().sky.shape[1::-1], 2: low_size(64, 40)}
    out = {key: 0 for key in ("input_deferred", "output_deferred", "state_chain", "in_place_then_frame", "writes_bound_result",
                              "pyramid_regrow", "two_meterings_rate_below_1")}
    sky_traced = {w: 0 for w in DISPLAY_WRITERS}
    deferred, chain, last_writer, write_at, bound_at, counted, pyramid = set(), set(), {}, {}, -1, set(), 0
    frames_after = np.cumsum([op[0] in ("frame", "dispatch") for op in program][::-1])[::-1]
    for i, op in enumerate(program):
        k = op[0]
        kinds[k] += 1
        result = tr.result if k != "dispatch" else op[1]
        reads, writes = display_reads_of(op, result), [t for t, _ in display_writes_of(op, result)]
        if k in DISPLAY_IMAGE_OPS:
            out["input_deferred"] += bool(deferred & set(reads))
            out["output_deferred"] += bool(deferred & set(writes) and frames_after[i] > 0)
            out["writes_bound_result"] += bool(tr.result in writes and frames_after[i] > 0)
        if k in ("tonemap", "bloom"):
            out["state_chain"] += bool(op[3] is not None and STATES[op[3]] in chain)
            following = [q[0] for q in program[i + 1:] if q[0] not in neutral][:1]
            out["in_place_then_frame"] += bool(op[1] == op[2] and following and following[0] in ("frame", "dispatch", "history"))
        if k == "bloom":
            need = pyramid_texels(*sizes[size_class(op[1])], op[4])
            out["pyramid_regrow"] += bool(0 < pyramid < need)
            pyramid = max(pyramid, need)
        if k == "meter":
            before = program[i - 1] if i else ("",)
            out["two_meterings_rate_below_1"] += bool(before[0] == "meter" and before[2] == op[2] and METER[before[4]]["rate"] < 1 and
                                                      METER[op[4]]["rate"] < 1 and size_class(before[1]) != size_class(op[1]))
        if k in ("frame", "dispatch") and tr.sky in last_writer and bound_at > write_at[tr.sky] and (tr.sky, write_at[tr.sky]) not in counted:
            counted.add((tr.sky, write_at[tr.sky]))
            if last_writer[tr.sky] in sky_traced:
                sky_traced[last_writer[tr.sky]] += 1
        # the state after the op
        if k == "meter":
            chain = (chain | {STATES[op[2]]}) if deferred & set(reads) else (chain - {STATES[op[2]]})
        elif k not in quiet + ("tonemap", "bloom"):
            chain = set()
        if k in ("frame", "dispatch"):
            deferred |= {t for t, _ in writes_of(op, result)}
        elif k not in quiet:
            deferred = set()
        for t, wk in display_writes_of(op, result):
            last_writer[t], write_at[t] = wk, i
        if k == "bind_sky":
            bound_at = i
        tr.apply(op)
    out["kinds"], out["written_then_sky_traced"] = kinds, sky_traced
    return out


def pipeline_coverage(program, nv=None):
    """Static facts about a program of the pipeline profile (tests/test_command_stream_model.py holds the seed set to them):
    kinds: op kind -> count;
    input_deferred: image operations that read a texture frames wrote while those frames could still be deferred;
    output_deferred: image operations that write such a texture, with a frame after them;
    vertex_write_in_batch: device-side vertex writes (skin, normals, set_device) with a dispatch before and after and nothing that
    submits in between;
    async_then_change: async queries followed by an in-place scene change before anything waits;
    mixed_readback: get_buffer of V / bounds over a range in which a device write and a host write have both landed since the scene was
    last prepared."""
    nv = len(pipeline_world()["rest_v"]) if nv is None else nv
    kinds = {k: 0 for k in PIPE_KINDS}
    tr = _PipeTrack()
    neutral = ("restart", "bind_sky", "bind_result", "camera")
    prepares = ("frame", "dispatch", "aov", "aov_into", "ray_query", "radiance_query", "radiance_pixels", "resample", "ray_query_async", "radiance_async")
    deferred, pending, write_open, async_open = set(), 0, False, False
    dev, host = np.zeros(nv, bool), np.zeros(nv, bool)
    out = {"input_deferred": 0, "output_deferred": 0, "vertex_write_in_batch": 0, "async_then_change": 0, "mixed_readback": 0}
    frames_after = np.cumsum([op[0] in ("frame", "dispatch") for op in program][::-1])[::-1]
    for i, op in enumerate(program):
        k = op[0]
        kinds[k] += 1
        result = tr.result if k != "dispatch" else op[1]
        if k in IMAGE_OPS:
            if deferred & set(pipeline_reads_of(op, result)):
                out["input_deferred"] += 1
            if deferred & {t for t, _ in pipeline_writes_of(op, result)} and frames_after[i] > 0:
                out["output_deferred"] += 1
        if k in ("get_buffer", "bounds"):
            a, n = (op[2], op[3]) if k == "get_buffer" else (op[1], op[2])
            if (k == "bounds" or op[1] == "V") and dev[a: a + n].any() and host[a: a + n].any():
                out["mixed_readback"] += 1
        if k in SCENE_CHANGES and async_open:
            out["async_then_change"] += 1
            async_open = False
        if k in OBSERVERS:
            async_open = False
        if k in ("ray_query_async", "radiance_async"):
            async_open = True
        if k in prepares:
            dev[:], host[:] = False, False
        if k in ("skin", "set_device"):
            a, n = (op[3], op[4]) if k == "skin" else (op[1], op[2])
            dev[a: a + n] = True
        elif k in ("set_host", "deform"):
            a, n = (op[1], op[2]) if k == "set_host" else (pipeline_world()["span"][0], pipeline_world()["span"][1] + 1)
            host[a: a + n] = True
        if k in ("frame", "dispatch"):
            if write_open:
                out["vertex_write_in_batch"] += 1
            write_open = False
            pending += 1
            deferred |= {t for t, _ in writes_of(op, result)}
        elif k in ("skin", "normals", "set_device"):
            write_open = pending > 0
        elif k in SCENE_CHANGES or k in ("snapshot", "ray_query_async", "radiance_async"):
            pass                                                 # (none of them submits the deferred frames)
        elif k not in neutral:
            pending, write_open, deferred = 0, False, set()
        tr.apply(op)
    out["kinds"] = kinds
    return out


def coverage(program):
    """Static facts about a program (tests/test_command_stream_model.py holds the seed set to them):
    kinds: op kind -> count;  sky_after: the writer kinds K for which a texture last written by K was bound as the sky AFTER that write and
    traced before anything else wrote it;  read_while_deferred: observers of an image reached while dispatches could still be deferred;
    edit_between_frames: scene edits with a dispatch before and after and nothing that submits in between."""
    kinds = {k: 0 for k in KINDS}
    tr = _Track()
    last_writer, write_at, bound_at = {}, {}, -1
    sky_after, read_deferred, edits = set(), 0, 0
    pending, edit_open = 0, False
    neutral = ("restart", "bind_sky", "bind_result", "camera")
    for i, op in enumerate(program):
        k = op[0]
        kinds[k] += 1
        if k in ("frame", "dispatch"):
            if tr.sky is not None and tr.sky in last_writer and bound_at > write_at[tr.sky]:
                sky_after.add(last_writer[tr.sky])
            if edit_open:
                edits += 1
            edit_open = False
            pending += 1
        elif k in ("move_mesh", "deform", "move_spheres"):
            edit_open = pending > 0
        elif k not in neutral:
            if k in ("get", "read_begin") and pending > 0:
                read_deferred += 1
            pending, edit_open = 0, False
        for t, w in writes_of(op, tr.result if k != "dispatch" else op[1]):
            last_writer[t], write_at[t] = w, i
        if k == "bind_sky":
            bound_at = i
        tr.apply(op)
    return {"kinds": kinds, "sky_after": sky_after, "read_while_deferred": read_deferred, "edit_between_frames": edits}


# ---- the sequential model -----------------------------------------------------------------------------------------------------------
def frame_uniforms_of(sc, frame):
    """(_PixelOffset, _Seed) RayTraceMaster.SetShaderParameters binds for its frame number `frame`."""
    if frame == 0:
        return (sc.pixel_offset[0], sc.pixel_offset[1]), sc.seed
    ox, oy, seed = scenes.frame_uniforms(frame, FRAME_SEED)
    return (ox, oy), seed


def encode(img, fmt):
    from unityraytracer_amd import host_io
    if fmt == "RGBA8_SRGB":
        return host_io.encode_srgb8(img)
    if fmt == "RGBA16F":
        with np.errstate(over="ignore"):
            return img.astype(np.float16)
    return img.copy()


def ray_hits(orc, o, d):
    """urt_RayHit of each ray as 12 float32 (distance, position, normal, then kind, object, primitive as int32 bits, u, v) from the oracle."""
    hit, nrm, _, ident = orc.aov(o, d)
    out = np.zeros((len(o), 12), F)
    out[:, 0], out[:, 1:4], out[:, 4:7] = hit[:, 3], hit[:, :3], nrm[:, :3]
    out[:, 7] = nrm[:, 3].astype(np.int32).view(F)
    out[:, 8:12] = ident
    return out


def run_model(program, width=64, height=40, bounces=2, threads=8, profile="frames", stats=None, stale_builds=(), world="mixed"):
    """-> (observations, final contents): observations is a list of (op index, kind, array | None), final a dict name -> array.
    profile="pipeline": the world and the ops of that profile (final holds the buffers too, under "V", "V.dev", ...: both sides of a
    buffer hold the same in program order); stats, a list, receives (op index, kind, figures) of the reproject / denoise / select /
    resample ops — what tests/test_command_stream_model.py measures non-vacuity on.
    profile="display": the world and the ops of that profile on top (final holds the exposure states "E0", "E1" and the master's "MS" as
    state_words, and "TM"; stats receives the figures of the upsample and meter ops, too).
    profile="dynamic": the world and the ops of that profile on top (final holds "DH" and both sides of W, LM, LS, HM, HS, the stride-28
    ones as heap_words; stats receives the figures of the morph and dof ops, too).  stale_builds: op indices of device builds that leave
    the heap and the leaves as they were — the non-vacuity probe of tests/test_command_stream_model.py, not a thing the library does.
    profile="solo": the dynamic profile's ops and motion_blur in the solo world (world="solo" goes with it; final holds neither LS nor HS:
    zero-count buffers do not exist; stats receives the figures of the motion_blur ops, too).  world="solo" under another profile: that
    profile's ops on the solo scene."""
    from oracle import pyoracle
    from reproject_ref import blit_add_history_ref
    assert profile in ("frames", "pipeline", "display", "dynamic", "solo"), profile
    world = "solo" if profile == "solo" else world
    solo = world == "solo"
    dynamic = profile in ("dynamic", "solo")
    display = profile == "display" or dynamic
    pipeline = profile == "pipeline" or display
    sc = make_scene(width, height, bounces, world)
    tex = {n: np.zeros((height, width, 4), F) for n in FRAME_TEX + (PIPE_TEX if pipeline else ()) + (UP_TEX + ("TM",) if display else ()) +
           (("DH",) if dynamic else ())}
    if dynamic:
        import dof_ref
        weights, master_dof = np.zeros(N_TARGETS, F), None
        leaves = [np.zeros(len(sc.mesh_objects), scenes.BVHNODE_DT), np.zeros(len(sc.spheres), scenes.BVHNODE_DT)]

        def device_build(i, kind, old):
            """The heap of `kind` built from the lists of sc; a stale build keeps the heap of the scene `old` (and the leaves)."""
            nonlocal sc
            sc = copy.copy(sc)
            if i in stale_builds:
                sc.mesh_bvh, sc.sphere_bvh = old.mesh_bvh, old.sphere_bvh
                return
            leaves[kind], heap = device_heap_of(sc, kind)
            setattr(sc, "sphere_bvh" if kind else "mesh_bvh", heap)

        def heap_buffers():
            return {"LM": leaves[0], "HM": sc.mesh_bvh} if solo else {"LM": leaves[0], "LS": leaves[1], "HM": sc.mesh_bvh, "HS": sc.sphere_bvh}
    if display:
        import bloom_ref
        import tonemap_ref
        import upsample_ref
        lw, lh = low_size(width, height)
        tex.update({n: np.zeros((lh, lw, 4), F) for n in LOW_TEX})
        states, master_bloom = {n: fresh_state() for n in STATES + ("MS",)}, False
    tex["S0"] = np.array(sc.sky, F)
    tex["S1"] = np.zeros_like(tex["S0"])
    sky, result, sample, frame, tickets, obs = "S0", "T0", 0, 0, [], []
    snap, p_scene, waiting = np.array(sc.vertices, F).reshape(-1, 3), sc, []
    stats = [] if stats is None else stats

    def oracle(num_rays=1):
        s = copy.copy(sc)
        s.sky = tex[sky] if sky is not None else np.zeros((1, 1, 4), F)        # an unbound texture reads zeros
        s.pixel_offset, s.seed = frame_uniforms_of(sc, frame)
        s.num_rays = num_rays
        return pyoracle.Oracle(s)

    def aov(frame_ray=False, size=None, sample_centres=False):
        from aov_ref import camera_rays
        orc = oracle()
        uniforms = (*frame_uniforms_of(sc, frame)[0], frame_uniforms_of(sc, frame)[1]) if frame_ray else None
        cam = orc.scene
        if sample_centres:                                       # RayTraceMaster._sample_centre_projection: the uv moved by half a pixel
            w, h = size or (width, height)
            p = np.array(cam.camera_inverse_projection, F).reshape(16).copy()
            p[12:16] += p[0:4] * F(1.0 / w) + p[4:8] * F(1.0 / h)
            cam = copy.copy(cam)
            cam.camera_inverse_projection = p
        O, D = camera_rays(cam, *(size or (width, height)), uniforms)
        return orc.aov(np.broadcast_to(O, D.shape), D)

    def exposure_of(k):
        return None if k is None else states[STATES[k] if k != "MS" else k]["exposure"]

    def tone_map(src, dst, k, op, exposure=1.0):
        tex[dst] = tonemap_ref.tonemap_ref(tex[src], exposure=exposure, op=TONEMAP_OPS.index(op), state_exposure=exposure_of(k))

    def bloom(src, dst, k, levels, flags=0):
        tex[dst] = bloom_ref.bloom_ref(tex[src], exposure=exposure_of(k), levels=levels, flags=flags)[0]

    for i, op in enumerate(program):
        k = op[0]
        if pipeline and k in OBSERVERS:                          # what the async queries answered is looked at now
            obs += waiting
            waiting = []
        if k == "motion_blur":
            import motion_blur_ref
            assert profile == "solo", op
            _, src, hit, dst, j = op
            out = motion_blur_ref.motion_blur_ref(tex[src], tex["MV"], tex[hit], **MBLUR[j])
            same_px = (out.view(np.uint32) == np.asarray(tex[src], F).view(np.uint32)).all(axis=-1)
            stats.append((i, k, {"changed": int((~same_px).sum()), "identical": int(same_px.sum())}))
            tex[dst] = out
            continue
        if dynamic and (k in DYNAMIC_KINDS or (k == "get_buffer" and op[1] in HEAP_BUFFERS)):
            if k == "morph":
                before = np.array(sc.vertices, F).reshape(-1, 3)
                weights = np.array(MORPH_WEIGHTS[op[1]], F)
                sc = edited_scene(sc, op, world)
                stats.append((i, k, {"moved": int((np.asarray(sc.vertices, F).reshape(-1, 3) != before).any(axis=1).sum())}))
            elif k == "device_heap":
                old = sc
                if op[1][0] == "morph":
                    weights = np.array(MORPH_WEIGHTS[op[1][1]], F)
                sc = edited_scene(sc, op[1], world)
                sc.mesh_bvh, sc.sphere_bvh = old.mesh_bvh, old.sphere_bvh      # the edit without its host SetData of the heap ...
                device_build(i, heap_kind(op[1]), old)                           # ... and the heap built where the buffers live
            elif k == "rebuild_heap":
                device_build(i, op[1], sc)
            elif k == "dof":
                _, src, hit, dst, j = op
                out = dof_ref.dof_ref(tex[src], tex[hit], **DOF[j])
                same_px = (out.view(np.uint32) == np.asarray(tex[src], F).view(np.uint32)).all(axis=-1)
                stats.append((i, k, {"changed": int((~same_px).sum()), "identical": int(same_px.sum())}))
                tex[dst] = out
            elif k == "master_dof":
                master_dof = op[1]
            elif k == "get_buffer":
                obs.append((i, k, heap_words(heap_buffers()[op[1]][op[2]: op[2] + op[3]])))
            continue
        if display and k in DISPLAY_KINDS:
            if k == "aov_low":
                tex["Lh"], tex["Lm"], tex["Lc"], tex["Li"] = aov(op[1], low_size(width, height))
            elif k == "upsample":
                _, color, count, with_low_count, flags = op
                out = upsample_ref.upsample_ref(*[tex[n] for n in ("Lc", "Lh", "Lm", "Li", "Gh", "Gn", "Gi")],
                                                low_count=tex["Ln"] if with_low_count else None,
                                                albedo=tex["Ga"] if flags & SKY_FROM_ALBEDO else None, flags=flags)
                tex[color] = out["color"]
                if count:
                    tex[count] = out["count"]
                stats.append((i, k, {"result": int(out["result"].sum()), "of": int(out["result"].size)}))
            elif k == "meter":
                name = STATES[op[2]]
                states[name] = tonemap_ref.auto_exposure_ref(tex[op[1]], tex["N"] if op[3] else None, states[name], **METER[op[4]])
                stats.append((i, k, {"counted": states[name]["counted"], "settled": states[name]["exposure"] == states[name]["target"]}))
            elif k == "tonemap":
                tone_map(*op[1:])
            elif k == "bloom":
                bloom(*op[1:])
            elif k == "state_get":
                obs.append((i, k, state_words(states[STATES[op[1]]])))
            elif k == "state_reset":
                states[STATES[op[1]]] = fresh_state()
            elif k == "master_bloom":
                master_bloom = op[1]
            elif k == "present_tm":                              # RayTraceMaster.ToneMap: the three explicit calls on the master's state
                dest = op[1] or "TM"
                states["MS"] = tonemap_ref.auto_exposure_ref(tex["C"], None, states["MS"], **MASTER_EXPOSURE)
                source = "C"
                if dynamic and master_dof is not None:           # the hit guide through the sample centres, then the blur into dest
                    tex["DH"] = aov(sample_centres=True)[0]
                    tex[dest] = dof_ref.dof_ref(tex["C"], tex["DH"], **DOF[master_dof])
                    source = dest
                if master_bloom:
                    bloom(source, dest, "MS", **MASTER_BLOOM)
                    source = dest
                tone_map(source, dest, "MS", op[2])
            continue
        if pipeline and k in NEW_KINDS + ("radiance_query",):
            if k == "aov":
                if op[1] == "P":
                    p_scene = sc
                for name, img in zip(aov_targets(op), aov(op[3])):
                    if name:
                        tex[name] = img
            elif k == "aov_into":
                tex[op[1]] = aov()[2]
            elif k == "reproject":
                from reproject_deform_ref import matrices_of, reproject_deformed_ref
                from reproject_motion_ref import reproject_objects_ref
                from reproject_ref import reproject_ref
                from unityraytracer_amd import host_scene
                _, form, j, max_history, src = op
                args = [tex[n] for n in (src, "N", "Ph", "Pn", "Pi", "Gh", "Gn", "Gi")]
                args += [scenes.world_to_clip(cameras(sc, world)[j], sc.camera_inverse_projection), sc.camera_to_world, sc.camera_inverse_projection]
                if form == "plain":
                    out = reproject_ref(*args, max_history=max_history)
                else:
                    tables = dict(mesh_motion=host_scene.mesh_motion(p_scene.mesh_objects, sc.mesh_objects),
                                  sphere_motion=None if solo else host_scene.sphere_motion(p_scene.spheres, sc.spheres))
                    if form == "objects":
                        out = reproject_objects_ref(*args, max_history=max_history, **tables)
                    else:
                        deform = (snap, sc.indices, matrices_of(p_scene.mesh_objects), pipeline_world(width, height, world)["deformed"])
                        out = reproject_deformed_ref(*args, max_history=max_history, deform=deform, **tables)
                tex["R"], tex["RN"], tex["MV"] = (np.ascontiguousarray(out[n], F) for n in ("color", "count", "motion"))
                stats.append((i, k, {"kept": float((tex["RN"][..., 0] > 0).mean()), "lost": float((tex["RN"][..., 0] == 0).mean())}))
            elif k == "denoise":
                from denoise_ref import denoise_ref, surface_mask
                _, src, iterations, albedo = op
                color, alb = np.asarray(tex[src], F), tex["Ga"] if albedo else None
                tex["D"] = denoise_ref(color, tex["Gh"], tex["Gn"], alb, iterations=iterations)          # float64: see the module's docstring
                moved = (tex["D"][..., :3] != color[..., :3].astype(np.float64)).any(axis=-1)
                stats.append((i, k, {"changed": int((moved & surface_mask(color, tex["Gh"], tex["Gn"], alb)).sum()), "identical": int((~moved).sum())}))
            elif k == "select":
                from resample_ref import select_pixels_ref
                xy = select_pixels_ref(tex[op[1]], op[2])
                stats.append((i, k, {"selected": len(xy), "of": width * height}))
                obs.append((i, k, xy))
            elif k == "resample":
                from resample_ref import blend_samples_ref, select_pixels_ref
                _, below, samples, max_history = op
                xy = select_pixels_ref(tex["N"], below)
                if len(xy):
                    img = oracle(samples).render(mode=0, threads=threads)
                    tex["H"], tex["N"] = blend_samples_ref(xy, img[xy[:, 1], xy[:, 0]], tex["H"], tex["N"], 1.0, max_history)
                stats.append((i, k, {"selected": len(xy), "of": width * height}))
                obs.append((i, k, np.array([len(xy)], np.int32)))
            elif k == "radiance_pixels":
                xy = query_xy(op[1], width, height)
                obs.append((i, k, oracle().render(mode=0, threads=threads)[xy[:, 1], xy[:, 0]]))
            elif k in ("radiance_query", "radiance_async"):
                o, d = query_rays(op[1])
                got = pyoracle.radiance(oracle(), pyoracle.path_rays(o, d, query_pixels(), 0.25), 1, bounces, threads=threads)
                (obs if k == "radiance_query" else waiting).append((i, k, got))
            elif k == "ray_query_async":
                waiting.append((i, k, ray_hits(oracle(), *query_rays(op[1]))))
            elif k in VERTEX_WRITES:
                sc = edited_scene(sc, op, world)
            elif k == "snapshot":
                snap = np.array(sc.vertices, F).reshape(-1, 3)
            elif k == "get_buffer":
                a = {"V": sc.vertices, "NB": sc.normals, "SNAP": snap}[op[1]]
                obs.append((i, k, np.array(np.asarray(a, F).reshape(-1, 3)[op[2]: op[2] + op[3]])))
            elif k == "bounds":
                import skin_ref
                lo3, hi3, n = skin_ref.bounds(sc.vertices, op[1], op[2])
                obs.append((i, k, np.concatenate([lo3, hi3, [F(n)]]).astype(F)))
            continue
        if k == "frame":
            tex[result] = oracle().render(mode=0, threads=threads)
            tex["C"] = pyoracle.accumulate(tex[result], tex["C"], float(sample))
            if op[1]:
                tex[op[1]] = tex["C"].copy()
            sample += 1
            frame += 1
        elif k == "dispatch":
            tex[op[1]] = oracle().render(mode=0, threads=threads)
            frame += 1
        elif k == "blit":
            tex[op[2]] = tex[op[1]].copy()
        elif k == "history":
            tex["H"], tex["N"] = blit_add_history_ref(tex[result], tex["H"], tex["N"], op[1])
        elif k == "setpixels":
            tex[op[1]] = np.full_like(tex[op[1]], F(op[2]))
        elif k == "restart":
            sample = 0
        elif k == "bind_sky":
            sky = op[1]
        elif k == "bind_result":
            result = "T1" if result == "T0" else "T0"
        elif k in ("move_mesh", "deform", "move_spheres", "camera"):
            sc = edited_scene(sc, op, world)
        elif k == "get":
            obs.append((i, k, tex[op[1]].copy()))
        elif k == "read_begin":
            tickets.append(encode(tex[op[1]], op[2]))
        elif k == "read_end":
            obs.append((i, k, tickets.pop(0)))
        elif k == "ray_query":
            o, d = query_rays(op[1])
            orc = oracle()
            out = np.zeros((N_QUERIES, 8), F)
            for j in range(N_QUERIES):
                r = orc.trace(o[j], d[j], mode=0)
                out[j, 0], out[j, 1:4], out[j, 4:7], out[j, 7] = r["distance"], r["position"], r["normal"], r["kind"]
            obs.append((i, k, out))
        elif k == "radiance_query":
            obs.append((i, k, None))
        elif k not in ("flush", "ptr"):
            raise ValueError(op)
    assert not tickets, "the program leaves a readback in flight"
    if pipeline:
        obs += waiting
        for name, a in (("V", sc.vertices), ("NB", sc.normals), ("SNAP", snap)):
            tex[name] = tex[name + ".dev"] = np.array(np.asarray(a, F).reshape(-1, 3))
    if display:
        tex.update({name: state_words(s) for name, s in states.items()})
    if dynamic:
        tex["W"] = tex["W.dev"] = weights
        for name, a in heap_buffers().items():
            tex[name] = tex[name + ".dev"] = heap_words(a)
    return obs, tex


# ---- the runner ---------------------------------------------------------------------------------------------------------------------
class _PipelineWorld:
    """The buffers and the plan the pipeline profile adds, on the GPU (pipeline_world holds their contents)."""

    def __init__(self, ctx, m, width, height, world="mixed"):
        from unityraytracer_amd.unity_api import ComputeBuffer
        w = pipeline_world(width, height, world)
        nv = len(w["rest_v"])
        self.made = []

        def buffer(count, stride, data=None):
            b = ComputeBuffer(ctx, count, stride)
            self.made.append(b)
            if data is not None:
                b.SetData(data)
            return b

        self.nv, self.ctx, self.ComputeBuffer = nv, ctx, ComputeBuffer
        self.V, self.NB = m._vertexBuffer, m._normalBuffer
        self.SNAP = buffer(nv, 12)
        self.SNAP.CopyFrom(self.V)                               # (from here on V has a device mirror: host SetData goes through the upload ring)
        self.skin = [buffer(nv, 12, w["rest_v"]), buffer(nv, 12, w["rest_n"]), buffer(nv, 16, w["bone_idx"]), buffer(nv, 16, w["bone_wgt"])]
        self.bones = [buffer(len(p), 48, p) for p in w["poses"]]
        self.mesh_motion = buffer(len(m.scene.mesh_objects), 48)
        self.sphere_motion = buffer(len(m.scene.spheres), 48) if len(m.scene.spheres) else None      # (a zero-count buffer does not exist)
        self.prev_objects, self.deformed = buffer(len(m.scene.mesh_objects), 112), buffer(len(m.scene.mesh_objects), 4, w["deformed"])
        lo, hi = w["span"]
        self.plan = ctx.normals_plan(self.V, m._indexBuffer, lo, hi - lo + 1)
        self.keep = []                                           # torch tensors the library may still read or write

    def both_sides(self, b, view=lambda raw: raw.view(F).reshape(-1, 3)):
        """(GetData of the whole buffer, what a device-to-device copy of it holds), each through `view`."""
        host = view(b.GetData())
        scratch = self.ComputeBuffer(self.ctx, b.count, b.stride)
        try:
            scratch.CopyFrom(b)
            return host, view(scratch.GetData())
        finally:
            scratch.Release()

    def release(self):
        if self.plan.handle:
            self.plan.Release()
        for b in self.made:
            b.Release()


class _DynamicWorld(_PipelineWorld):
    """... and what the dynamic profile adds (dynamic_world holds the contents): the morph plan, W, the leaf buffers, and the two bound
    heap buffers under their names."""

    def __init__(self, ctx, m, width, height, world="mixed"):
        super().__init__(ctx, m, width, height, world)
        w = dynamic_world(width, height, world)
        lo, hi = w["span"]
        self.morph_plan = ctx.morph_plan(w["deltas"], N_TARGETS, lo, hi - lo + 1)
        n = w["counts"]
        self.W = self.made_buffer(N_TARGETS, 4, np.zeros(N_TARGETS, F))
        self.LM = self.made_buffer(n["LM"], 28, np.zeros(n["LM"], scenes.BVHNODE_DT))
        self.LS = self.made_buffer(n["LS"], 28, np.zeros(n["LS"], scenes.BVHNODE_DT)) if n["LS"] else None
        self.HM, self.HS = m._meshObjectBVHBuffer, m._sphereBVHBuffer
        assert (self.HM.count, self.HS.count if self.HS is not None else 0) == (n["HM"], n["HS"])

    def made_buffer(self, count, stride, data):
        b = self.ComputeBuffer(self.ctx, count, stride)
        self.made.append(b)
        b.SetData(data)
        return b

    def device_build(self, m, kind):
        """The heap of kind 0 | 1 built where the buffers live: leaf boxes, then the heap into the bound heap buffer's device side."""
        if kind == 0:
            self.ctx.mesh_leaf_bounds(m._meshObjectBuffer, self.V, m._indexBuffer, self.LM)
            self.ctx.build_object_bvh(self.LM, self.HM)
        else:
            self.ctx.sphere_leaf_bounds(m._sphereBuffer, self.LS)
            self.ctx.build_object_bvh(self.LS, self.HS)

    def release(self):
        if self.morph_plan.handle:
            self.morph_plan.Release()
        super().release()


OPTION_DEFAULTS = {"tile_entry": -1, "refit": 1, "prepare_device": 0}      # the library's defaults of the options run_gpu's `options` may name


def run_gpu(ctx, program, frames_per_launch, overlap_launches, width=64, height=40, bounces=2, profile="frames", probe=None, world="mixed",
            options=None):
    """The program through the Python API -> (observations, final contents, counters, [(op index, launch_info()) after every op of SUBMITTING]
    — profile="solo": after every op outside SOLO_QUIET, and (-1, launch_info()) at the end).
    probe(op index, op, master, the pipeline profile's buffers | None) is called after every op: for protocols that look at the
    library's own bookkeeping (it must not call anything that submits or waits, or the run is no longer the program's).
    profile="display": as in run_model; the states are read at the end through Context.exposure_state.
    profile="dynamic": as in run_model (the probe's last argument is then a _DynamicWorld, with W, LM, LS, HM and HS).
    profile="solo" / world: as in run_model (LS and HS are None then).  options: {name of OPTION_DEFAULTS: value}, set behind the three
    options every run sets and put back to the library's defaults at the end."""
    from unityraytracer_amd import Graphics, RayTraceMaster, RenderTexture
    assert profile in ("frames", "pipeline", "display", "dynamic", "solo"), profile
    world = "solo" if profile == "solo" else world
    solo = world == "solo"
    dynamic = profile in ("dynamic", "solo")
    display = profile == "display" or dynamic
    pipeline = profile == "pipeline" or display
    options = dict(options or {})
    assert set(options) <= set(OPTION_DEFAULTS), options
    ctx.set_option("kernel_mode", 3)
    ctx.set_option("frames_per_launch", frames_per_launch)
    ctx.set_option("overlap_launches", overlap_launches)
    m, tex, pw = None, {}, None
    try:
        for name, value in options.items():
            ctx.set_option(name, value)
        sc = make_scene(width, height, bounces, world)
        m = RayTraceMaster(ctx, sc, frame_seed=FRAME_SEED)
        for n in FRAME_TEX + (PIPE_TEX if pipeline else ()) + (UP_TEX if display else ()):
            tex[n] = RenderTexture(ctx, width, height)
        for n in LOW_TEX if display else ():
            tex[n] = RenderTexture(ctx, *low_size(width, height))
        m._target, m._converged = tex["T0"], tex["C"]
        m._bind_for_queries()                                  # buffers, the scene's sky, the bindings
        tex["S0"] = m.SkyboxTexture
        tex["S1"] = RenderTexture(ctx, tex["S0"].width, tex["S0"].height)
        sh = m.RayTraceShader
        if pipeline:
            import torch
            from unityraytracer_amd import host_scene
            pw = (_DynamicWorld if dynamic else _PipelineWorld)(ctx, m, width, height, world)
            dev = torch.device("cuda", ctx.device)
            bufs = {"V": pw.V, "NB": pw.NB, "SNAP": pw.SNAP}
            heap_bufs = {n: getattr(pw, n) for n in HEAP_BUFFERS if getattr(pw, n) is not None} if dynamic else {}
        if display:
            states = [torch.zeros(STATE_WORDS, dtype=torch.int32, device=dev) for _ in STATES]
            m.EnableAutoExposure(**MASTER_EXPOSURE)
        p_scene, waiting = m.scene, []
        ctx.reset_counters()
        obs, infos, tickets = [], [], []
        gx, gy = (width + 7) // 8, (height + 7) // 8

        def drain():
            if waiting:
                ctx.synchronize()
                torch.cuda.synchronize(dev)
                for j, kind, out, _ in waiting:
                    obs.append((j, kind, out.cpu().numpy()))
                del waiting[:]

        def vertex_edit(op, host_heap=True):
            """An op of VERTEX_WRITES or a morph, with (the ops as the older profiles know them) or without the host SetData of the heap."""
            k = op[0]
            new = edited_scene(m.scene, op, world)
            if k == "skin":
                ctx.skin_vertices(*pw.skin, pw.bones[op[1]], op[3], op[4], pw.V, pw.NB if op[2] else None)
            elif k == "normals":
                pw.plan.compute(pw.NB)
            elif k == "morph":
                pw.W.SetData(np.array(MORPH_WEIGHTS[op[1]], F))
                pw.morph_plan.morph(pw.skin[0], pw.skin[1] if op[2] else None, pw.W, pw.V, pw.NB if op[2] else None, op[3])
            else:
                part = np.ascontiguousarray(np.asarray(new.vertices, F).reshape(-1, 3)[op[1]: op[1] + op[2]])
                if k == "set_device":
                    t = torch.from_numpy(part).to(dev)
                    pw.keep.append(t)                    # (the copy is only enqueued)
                    pw.V.SetDataDevice(t, op[1], op[2])
                else:
                    pw.V.SetData(part, 0, op[1], op[2])
            if k != "normals" and host_heap:
                m._meshObjectBVHBuffer.SetData(new.mesh_bvh)
            m.scene = new

        def object_edit(op, host_heap=True):
            """move_mesh, deform, move_spheres or camera, likewise."""
            k = op[0]
            new = edited_scene(m.scene, op, world)
            if k == "move_mesh":
                m._meshObjectBuffer.SetData(new.mesh_objects)
            elif k == "deform":
                lo, hi = blob_span(new)
                m._vertexBuffer.SetData(np.ascontiguousarray(new.vertices[lo: hi + 1]), 0, lo, hi - lo + 1)
            elif k == "move_spheres":
                m._sphereBuffer.SetData(new.spheres)
            if host_heap and k in ("move_mesh", "deform"):
                m._meshObjectBVHBuffer.SetData(new.mesh_bvh)
            elif host_heap and k == "move_spheres":
                m._sphereBVHBuffer.SetData(new.sphere_bvh)
            m.scene = new

        for i, op in enumerate(program):
            k = op[0]
            if profile == "solo" and i and program[i - 1][0] not in SOLO_QUIET + SUBMITTING:
                infos.append((i - 1, ctx.launch_info()))         # (the op before this one has submitted what was deferred: asking changes nothing)
            if pipeline and k in OBSERVERS:
                drain()
            if k == "motion_blur":
                assert profile == "solo", op
                ctx.motion_blur(tex[op[1]], tex["MV"], tex[op[2]], tex[op[3]], **MBLUR[op[4]])
                if probe:
                    probe(i, op, m, pw)
                continue
            if dynamic and (k in DYNAMIC_KINDS or (k == "get_buffer" and op[1] in HEAP_BUFFERS)):
                if k == "morph":
                    vertex_edit(op)
                elif k == "device_heap":
                    (vertex_edit if op[1][0] in VERTEX_WRITES + ("morph",) else object_edit)(op[1], host_heap=False)
                    pw.device_build(m, heap_kind(op[1]))
                elif k == "rebuild_heap":
                    pw.device_build(m, op[1])
                elif k == "dof":
                    ctx.depth_of_field(tex[op[1]], tex[op[2]], tex[op[3]], **DOF[op[4]])
                elif k == "master_dof":
                    m.EnableDepthOfField(**DOF[op[1]]) if op[1] is not None else m.DisableDepthOfField()
                elif k == "get_buffer":
                    obs.append((i, k, heap_words(heap_bufs[op[1]].GetData(op[2], op[3]))))
                if probe:
                    probe(i, op, m, pw)
                continue
            if display and k in DISPLAY_KINDS:
                state = states[op[3]] if k in ("tonemap", "bloom") and op[3] is not None else None
                if k == "aov_low":
                    m.SetShaderParameters()
                    ctx.render_aov(tex["Lh"], tex["Lm"], tex["Lc"], tex["Li"], frame_ray=op[1])
                elif k == "upsample":
                    _, color, count, with_low_count, flags = op
                    ctx.upsample(*[tex[n] for n in ("Lc", "Lh", "Lm", "Li", "Gh", "Gn", "Gi")], tex[color], tex[count] if count else None,
                                 low_count=tex["Ln"] if with_low_count else None, albedo=tex["Ga"] if flags & SKY_FROM_ALBEDO else None,
                                 wide_fallback=bool(flags & WIDE_FALLBACK), sky_from_albedo=bool(flags & SKY_FROM_ALBEDO))
                elif k == "meter":
                    ctx.auto_exposure(tex[op[1]], states[op[2]], tex["N"] if op[3] else None, **METER[op[4]])
                elif k == "tonemap":
                    ctx.tonemap(tex[op[1]], tex[op[2]], state, op=op[4], exposure=op[5])
                elif k == "bloom":
                    ctx.bloom(tex[op[1]], tex[op[2]], state, levels=op[4], flags=op[5])
                elif k == "state_get":
                    obs.append((i, k, state_words(ctx.exposure_state(states[op[1]]))))
                elif k == "state_reset":
                    # The library orders torch's stream in front of its own (unity_api._sync_torch_stream), not the other way round: a
                    # caller that writes a state with torch waits for the library first.  That wait is part of the op, in the model too
                    # (it submits the deferred frames: the op is one of SUBMITTING).
                    ctx.synchronize()
                    states[op[1]].zero_()
                    infos.append((i, ctx.launch_info()))
                elif k == "master_bloom":
                    m.EnableBloom(**MASTER_BLOOM) if op[1] else m.DisableBloom()
                elif k == "present_tm":
                    m.ToneMap(tex[op[1]] if op[1] else None, op[2])
                if probe:
                    probe(i, op, m, pw)
                continue
            if pipeline and k in NEW_KINDS:
                if k == "aov":
                    if op[1] == "P":
                        p_scene = m.scene
                    m.SetShaderParameters()
                    ctx.render_aov(*[tex[t] if t else None for t in aov_targets(op)], frame_ray=op[3])
                elif k == "aov_into":
                    m.SetShaderParameters()
                    ctx.render_aov(albedo=tex[op[1]])
                elif k == "reproject":
                    _, form, j, max_history, src = op
                    m.SetShaderParameters()
                    extra = {}
                    if form != "plain":
                        pw.mesh_motion.SetData(host_scene.mesh_motion(p_scene.mesh_objects, m.scene.mesh_objects))
                        extra = dict(mesh_motion=pw.mesh_motion)
                        if pw.sphere_motion is not None:
                            pw.sphere_motion.SetData(host_scene.sphere_motion(p_scene.spheres, m.scene.spheres))
                            extra["sphere_motion"] = pw.sphere_motion
                    if form == "deformed":
                        pw.prev_objects.SetData(p_scene.mesh_objects)
                        extra["deform"] = (pw.SNAP, m._indexBuffer, pw.prev_objects, pw.deformed)
                    ctx.reproject(*[tex[n] for n in (src, "N", "Ph", "Pn", "Pi", "Gh", "Gn", "Gi", "R", "RN")],
                                  scenes.world_to_clip(cameras(m.scene, world)[j], m.scene.camera_inverse_projection), motion=tex["MV"],
                                  max_history=max_history, **extra)
                elif k == "denoise":
                    ctx.denoise(tex[op[1]], tex["D"], tex["Gh"], tex["Gn"], tex["Ga"] if op[3] else None, iterations=op[2])
                elif k == "select":
                    obs.append((i, k, ctx.select_pixels(tex[op[1]], op[2]).cpu().numpy()))
                elif k == "resample":
                    m.SetShaderParameters()
                    sh.SetTexture(0, "Result", m._target)
                    obs.append((i, k, np.array([ctx.resample_below(tex["H"], tex["N"], op[1], op[2], bounces, 1.0, op[3])], np.int32)))
                elif k == "radiance_pixels":
                    m.SetShaderParameters()
                    sh.SetTexture(0, "Result", m._target)
                    obs.append((i, k, ctx.radiance_query_pixels(query_xy(op[1], width, height), 1, bounces)))
                elif k in ("ray_query_async", "radiance_async"):
                    m.SetShaderParameters()
                    o, d = query_rays(op[1])
                    if k == "ray_query_async":
                        rays = np.concatenate([o, np.full((N_QUERIES, 1), np.inf, F), d, np.zeros((N_QUERIES, 1), F)], axis=1)
                    else:
                        from oracle import pyoracle
                        rays = pyoracle.path_rays(o, d, query_pixels(), 0.25)
                    d_rays = torch.from_numpy(np.ascontiguousarray(rays, F)).to(dev)
                    d_out = torch.zeros((N_QUERIES, 12 if k == "ray_query_async" else 4), dtype=torch.float32, device=dev)
                    torch.cuda.synchronize(dev)                  # the tensors are written on torch's stream, the query runs on the library's
                    if k == "ray_query_async":
                        ctx.check(ctx.lib.urt_ray_query_device(ctx._h, d_rays.data_ptr(), N_QUERIES, d_out.data_ptr(), 0))
                    else:
                        ctx.check(ctx.lib.urt_radiance_query_device(ctx._h, d_rays.data_ptr(), N_QUERIES, 1, bounces, d_out.data_ptr(), 0))
                    waiting.append((i, k, d_out, d_rays))        # not waited for
                elif k in VERTEX_WRITES:
                    vertex_edit(op)
                elif k == "snapshot":
                    pw.SNAP.CopyFrom(pw.V)
                elif k == "get_buffer":
                    obs.append((i, k, bufs[op[1]].GetData(op[2], op[3]).view(F).reshape(-1, 3)))
                elif k == "bounds":
                    lo3, hi3, n = ctx.buffer_bounds(pw.V, op[1], op[2])
                    obs.append((i, k, np.concatenate([lo3, hi3, [F(n)]]).astype(F)))
                if probe:
                    probe(i, op, m, pw)
                continue
            if k == "frame":
                m.OnRenderImage(tex[op[1]] if op[1] else None)
            elif k == "dispatch":
                m.SetShaderParameters()
                sh.SetTexture(0, "Result", tex[op[1]])
                sh.Dispatch(0, gx, gy, 1)
                m._frame += 1
            elif k == "blit":
                Graphics.Blit(tex[op[1]], tex[op[2]])
            elif k == "history":
                ctx.blit_add_history(m._target, tex["H"], tex["N"], op[1])
            elif k == "setpixels":
                t = tex[op[1]]
                t.SetPixels(np.full((t.height, t.width, 4), op[2], F))
            elif k == "restart":
                m._currentSample = 0
            elif k == "bind_sky":
                m.SkyboxTexture = tex[op[1]] if op[1] else None
                sh.SetTexture(0, "_SkyboxTexture", m.SkyboxTexture)
            elif k == "bind_result":
                m._target = tex["T1"] if m._target is tex["T0"] else tex["T0"]
            elif k in ("move_mesh", "deform", "move_spheres", "camera"):
                object_edit(op)
            elif k == "flush":
                ctx.flush()
            elif k == "ptr":
                assert tex[op[1]].device_ptr()
            elif k == "get":
                obs.append((i, k, (m._tonemapped if op[1] == "TM" else tex[op[1]]).GetPixels()))
            elif k == "read_begin":
                tickets.append((tex[op[1]], tex[op[1]].ReadBegin(op[2])))
            elif k == "read_end":
                t, ticket = tickets.pop(0)
                obs.append((i, k, t.ReadEnd(ticket)))
            elif k == "ray_query":
                m.SetShaderParameters()
                o, d = query_rays(op[1])
                h = ctx.ray_query(o, d)
                out = np.zeros((N_QUERIES, 8), F)
                out[:, 0], out[:, 1:4], out[:, 4:7], out[:, 7] = h["distance"], h["position"], h["normal"], h["kind"]
                obs.append((i, k, out))
            elif k == "radiance_query":
                m.SetShaderParameters()
                o, d = query_rays(op[1])
                obs.append((i, k, ctx.radiance_query(o, d, query_pixels(), 0.25, 1, bounces)))
            else:
                raise ValueError(op)
            if k in SUBMITTING:                                  # (launch_info() submits what is deferred: asked only where the op has done so)
                infos.append((i, ctx.launch_info()))
            if probe:
                probe(i, op, m, pw)
        while tickets:                                           # (a program ends its own readbacks; this is for one that failed half-way)
            t, ticket = tickets.pop(0)
            t.ReadEnd(ticket)
        if pipeline:
            drain()
        final = {n: t.GetPixels() for n, t in tex.items()}
        if profile == "solo":                                    # (everything is submitted: the last launch of the run, under the index -1)
            infos.append((-1, ctx.launch_info()))
        if pipeline:
            for name, b in bufs.items():
                final[name], final[name + ".dev"] = pw.both_sides(b)
        if display:
            final["TM"] = m._tonemapped.GetPixels() if m._tonemapped is not None else np.zeros((height, width, 4), F)
            for name, t in zip(STATES + ("MS",), states + [m._exposureState]):
                final[name] = state_words(ctx.exposure_state(t))
        if dynamic:
            final["DH"] = m._dofHit.GetPixels() if m._dofHit is not None else np.zeros((height, width, 4), F)
            final["W"], final["W.dev"] = pw.both_sides(pw.W, lambda raw: raw.view(F).reshape(-1))
            for name, b in heap_bufs.items():
                final[name], final[name + ".dev"] = pw.both_sides(b, heap_words)
        return obs, final, ctx.counters(), infos
    finally:
        ctx.set_option("frames_per_launch", 0)
        ctx.set_option("overlap_launches", 1)
        for name in options:
            ctx.set_option(name, OPTION_DEFAULTS[name])
        if pw is not None:
            ctx.synchronize()                                    # (nothing enqueued still reads a tensor or a buffer of this run)
            pw.release()
        if m is not None:
            for t in tex.values():
                if t.handle:
                    t.Release()
            for name in ("_target", "_converged", "SkyboxTexture"):      # the master releases none of them twice
                t = getattr(m, name)
                if t is not None and not t.handle:
                    setattr(m, name, None)
            m.OnDisable()


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
def same(a, b):
    """Bit for bit (NaNs of any payload count as equal, as in tests/test_gpu_ray_query.py).  A float64 `b` is the model's denoised image
    (tests/denoise_ref.py is the float64 formula): there `a` is held to what include/urt.h promises of urt_denoise, |a - b| <= 1e-4 (1 + |b|)
    per colour channel, and to alpha bit for bit."""
    if a is None or b is None:
        return a is None and b is None
    if b.dtype == np.float64 and a.dtype == np.float32 and a.shape == b.shape:
        with np.errstate(invalid="ignore"):
            close = (np.abs(a[..., :3] - b[..., :3]) <= 1e-4 * (1.0 + np.abs(b[..., :3]))) | (np.isnan(a[..., :3]) & np.isnan(b[..., :3]))
        return bool(close.all()) and same(a[..., 3], b[..., 3].astype(np.float32))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


def first_difference(got, want, radiance=True):
    """None, or (index of the op up to which the program matters | None = all of it, what differs first): observations in order, then the
    final contents.  radiance=False leaves the recorded radiance queries out (the model has none)."""
    obs_a, fin_a = got[0], got[1]
    obs_b, fin_b = want[0], want[1]
    if len(obs_a) != len(obs_b):
        return None, f"{len(obs_a)} observations against {len(obs_b)}"
    for n, ((i, k, a), (j, k2, b)) in enumerate(zip(obs_a, obs_b)):
        if (i, k) != (j, k2):
            return i, f"observation {n} is {k} of op {i} against {k2} of op {j}"
        if k == "radiance_query" and not radiance:
            continue
        if not same(a, b):
            bad = int(np.count_nonzero(a.reshape(-1) != b.reshape(-1))) if a.shape == b.shape else -1
            return (None if k.endswith("_async") else i), f"observation {n} ({k}, op {i}) differs in {bad} of {a.size} values"
    for name in fin_b:
        if not same(fin_a[name], fin_b[name]):
            return None, f"final contents of {name} differ in {int(np.count_nonzero(fin_a[name] != fin_b[name]))} of {fin_a[name].size} values"
    return None


def describe(program, upto=None):
    ops = program if upto is None else program[: upto + 1]
    return "\n".join(f"  {i:3d} {op}" for i, op in enumerate(ops))
