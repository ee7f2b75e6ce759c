/* urt.h — C ABI of libunityraytracer_amd.so: the MI355X (gfx950) replacement for the GPU calls that
 * RemyMuj/UnityRayTracer's Assets/Scripts/RayTraceMaster.cs ("RM") makes through UnityEngine:
 * ComputeBuffer / ComputeShader.Set* / ComputeShader.Dispatch / RenderTexture / Graphics.Blit.
 * Each entry point cites the reference call site it stands in for; the C# P/Invoke shim that binds
 * them is shown in INTEGRATION.md.  The kernels behind urt_shader_dispatch()/urt_blit_add() are
 * hand-written HIP restatements of Assets/Shaders/RayTraceShader.compute ("RS", kernel CSMain) and
 * Assets/Shaders/AdditionShader.shader ("AS").
 *
 * Conventions:
 *  - plain C types only; every function returns an int status (URT_OK == 0) and never unwinds;
 *    urt_last_error() returns the message for the last non-zero status (Unity's API returns void
 *    and logs — a caller that wants that behaviour logs the string and carries on);
 *  - host memory passed in is copied before the call returns (ComputeBuffer.SetData semantics);
 *  - handles are opaque 64-bit ids owned by the library until *_release();
 *  - one caller thread per context (Unity main thread); work is issued in order on one HIP stream,
 *    so no synchronisation is needed between dispatch and blit; urt_synchronize() or a readback
 *    waits for completion.  The context-free urt_host_* helpers may be called from any thread
 *    concurrently: each thread has its own last-error strings;
 *  - buffer layouts are the byte layouts of urt_types.h (RM:42-45), matrices are 16 floats in
 *    Unity Matrix4x4 memory order (column-major), images are RGBA32F with row 0 = bottom row
 *    (RS:434,468: id.y = 0 is uv.y = -1);
 *  - there is no CPU fallback: every entry point that needs the GPU fails with
 *    URT_ERR_NO_DEVICE if no HIP device is usable.
 */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "urt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define URT_API __attribute__((visibility("default")))

typedef struct urt_context urt_context;
typedef uint64_t urt_handle;

enum {
  URT_OK = 0,
  URT_ERR_INVALID_ARGUMENT = 1,
  URT_ERR_INVALID_HANDLE = 2,
  URT_ERR_NO_DEVICE = 3,
  URT_ERR_HIP = 4,
  URT_ERR_UNBOUND = 5,        /* dispatch without a Result texture / camera matrices */
  URT_ERR_LAYOUT = 6,         /* stride/count does not match the layout the name requires */
  URT_ERR_OUT_OF_MEMORY = 7,
  URT_ERR_SCENE = 8,          /* scene data fails validation (index out of range, stack too deep) */
  URT_ERR_WATCHDOG = 9        /* waves of a trace launch left through the kernel's iteration cap: pixels are missing.  Reported
                                 once, by the first urt_synchronize / urt_texture_get_pixels after the launch completed */
};

/* ---- library / context ------------------------------------------------------------------- */
URT_API int urt_abi_version(void);                       /* bumps when this header changes incompatibly (still 4: the ray queries,
                                                            the feature buffers, the denoiser, the temporal reprojection, the
                                                            resampling, the ranged SetData and the device side of the buffers —
                                                            urt_buffer_set_data_device, urt_buffer_get_data_range,
                                                            urt_skin_vertices, urt_buffer_bounds, urt_debug_buffer_state — the
                                                            normals on the device, urt_buffer_copy, urt_reproject_deformed,
                                                            urt_upsample, urt_auto_exposure, urt_tonemap, urt_bloom,
                                                            urt_depth_of_field and the blend shapes on the device —
                                                            urt_morph_plan_create, urt_morph_plan_info, urt_morph_plan_release,
                                                            urt_morph_vertices, urt_debug_build_morph_plan —
                                                            and the object-level BVH on the device —
                                                            urt_mesh_leaf_bounds_device, urt_sphere_leaf_bounds_device,
                                                            urt_build_object_bvh_device — were added without changing anything
                                                            that existed) */
URT_API int urt_device_count(int* out_count);
/* One context per process and GPU (the one-process-per-GPU model).  device = HIP ordinal. */
URT_API int urt_context_create(int device, urt_context** out_ctx);
URT_API int urt_context_destroy(urt_context* ctx);
/* Message for the last failing call on ctx (ctx may be NULL for create failures). Never NULL. */
URT_API const char* urt_last_error(urt_context* ctx);
/* Issue all work on a caller-owned hipStream_t (e.g. torch's current stream); NULL = own stream. */
URT_API int urt_context_set_stream(urt_context* ctx, void* hip_stream);
/* Block until everything issued so far is complete. */
URT_API int urt_synchronize(urt_context* ctx);
/* Frame batching.  On its own stream the library DEFERS urt_shader_dispatch (default kernel) and the urt_blit_add /
 * urt_blit / urt_texture_pack_rows calls that follow it, and traces several consecutive frames with one persistent launch
 * (a 1080p frame is too small to fill 256 CUs through its 8-bounce tail; "frames_per_launch" below).  The whole frame of
 * RM:806-820 — Dispatch, Blit(_target, _converged, mat), Blit(_converged, destination) — is deferred; the blends of a batch
 * and the present run as ONE pass after the launch.  Every call that could observe an image (readback, synchronize,
 * counters, SetPixels, release, a device pointer handed out, option changes, ...) submits the deferred work first, so
 * results and ordering are exactly those of immediate execution (RM:806-820 is in-order).
 * As-if rule for the present: a deferred urt_blit(src, dst) that is followed by another deferred urt_blit to the same dst,
 * with nothing that could observe dst in between, is not materialised — dst receives the later image only.  No observer
 * can tell (observers submit first); a caller that looks at dst's memory by its own means must call urt_flush /
 * urt_synchronize first, as for any deferred work.
 * An error of deferred work (a failing launch) is reported by the call that submits it.
 * urt_flush submits the deferred work to the stream without waiting — for callers that synchronise by their own means
 * (their own stream + events); with a caller-owned stream deferral is off unless "frames_per_launch" is set explicitly. */
URT_API int urt_flush(urt_context* ctx);

/* ---- ComputeBuffer ------------------------------------------------------------------------ */
/* new ComputeBuffer(count, stride)                                   RM:247 */
URT_API int urt_buffer_create(urt_context* ctx, int count, int stride, urt_handle* out_buffer);
/* buffer.SetData(List<T>) — synchronous copy of count*stride bytes   RM:250 */
URT_API int urt_buffer_set_data(urt_context* ctx, urt_handle buffer, const void* data, int count);
/* buffer.SetData(data, managedStart, computeStart, count): elements first .. first+count-1 (Unity's ranged overload).  `data` points at
 * the first of the `count` elements and is copied before the call returns; elements of a buffer that were never set read as zero bytes.
 * count == 0 changes nothing; data equal to what the buffer holds dirties nothing, as with urt_buffer_set_data.
 * URT_ERR_INVALID_ARGUMENT (nothing is written): first < 0, count < 0, first + count beyond the buffer, NULL data with count > 0. */
URT_API int urt_buffer_set_data_range(urt_context* ctx, urt_handle buffer, int first, const void* data, int count);
/* buffer.count / buffer.stride                                       RM:237 */
URT_API int urt_buffer_get_info(urt_context* ctx, urt_handle buffer, int* out_count, int* out_stride);
/* buffer.Release()                                                   RM:195-210, 238 */
URT_API int urt_buffer_release(urt_context* ctx, urt_handle buffer);

/* ---- the device side of a ComputeBuffer ------------------------------------------------------------------------------------------
 * A buffer is a host copy; the first device-side use below gives it a DEVICE MIRROR of count * stride bytes, filled from the host copy
 * and from then on kept current: a host SetData pushes what it changed, in stream order.  The writers below leave the HOST copy behind
 * instead: the elements they wrote are STALE on the host until something reads them there — urt_buffer_get_data_range, a full scene
 * preparation, the small scene tables, a motion table — which first downloads them (a synchronising device-to-host copy, counted by
 * urt_debug_buffer_state).  A host SetData never downloads for its compare: elements inside the stale range count as differing and
 * leave it (when that would split the range, the part behind the written elements is downloaded first).
 * When _Vertices / _Normals were written on the device and the change is one the scene takes in place (option "refit_vertices"), the
 * dirty elements reach the scene's copies by a device-to-device copy on the context's stream: no host copy, no upload, no download.
 * A full preparation (for whatever reason: _Indices rewritten, buffers of another count bound, "refit" / "refit_vertices" off, a rebuild
 * forced by "refit_rebuild_pct") sees the device-written data through the download by default.  With option "prepare_device" = 1 it takes
 * _Vertices / _Indices / _Normals from their mirrors instead — a device-to-device copy on the context's stream into the scene's own copies,
 * a build on the GPU, the MeshObjects' vertex spans found on the GPU (csrc/index_span.hip): none of the three is downloaded, their stale
 * ranges stay, and a buffer that was only ever written on the device needs no host SetData at all.  The small tables (_MeshObjects,
 * _MeshBVH, _Spheres, _SphereBVH) are packed on the host either way and come down first when they were written on the device.
 * urt_buffer_release and urt_context_destroy give the mirror back.  There are no urt_group_* twins of the calls of this section: a group
 * host reaches the ranks' contexts through urt_group_context. */
/* Ranged SetData whose source is DEVICE memory (4-byte aligned): the copy is enqueued on the context's stream and the call returns
 * without synchronising; the source is read in stream order and the caller orders its producer, as with urt_ray_query_device.  Every
 * element of the range counts as changed (no compare); bound slots are dirtied exactly as by urt_buffer_set_data_range.  Works for a
 * buffer of any stride; only _Vertices / _Normals have the in-place path, for other bound slots the next preparation downloads.
 * count == 0 changes nothing.  Checked first, nothing enqueued: unknown handle URT_ERR_INVALID_HANDLE; first < 0, count < 0, a range
 * beyond the buffer, NULL or misaligned d_data with count > 0 URT_ERR_INVALID_ARGUMENT. */
URT_API int urt_buffer_set_data_device(urt_context* ctx, urt_handle buffer, int first, const void* d_data, int count);
/* ComputeBuffer.GetData: the buffer's current contents, elements first .. first+count-1, into host memory; downloads stale elements
 * (synchronises).  Elements that were never set read as zero bytes.  Errors as urt_buffer_set_data_range. */
URT_API int urt_buffer_get_data_range(urt_context* ctx, urt_handle buffer, int first, void* out, int count);
/* A snapshot that stays on the device: elements src_first .. src_first+count-1 of src's mirror are copied to elements dst_first ..
 * dst_first+count-1 of dst's mirror (both buffers get mirrors, as with every first device-side use).  The copy is enqueued on the
 * context's stream; nothing is synchronised and nothing is downloaded.  The destination range becomes stale and dirty as a whole,
 * exactly as with urt_buffer_set_data_device.  A source whose host copy is the current one is read from its mirror, which is current by
 * the rule above; a source written on the device is read where it was written.  (urt_reproject_deformed reads the previous vertex
 * positions of a deforming mesh from such a snapshot of _Vertices.)
 * Checked first, nothing enqueued: a handle that is 0 or unknown URT_ERR_INVALID_HANDLE; strides that differ, a negative first or count,
 * a range outside either buffer, src == dst URT_ERR_INVALID_ARGUMENT.  count == 0 returns URT_OK after the checks. */
URT_API int urt_buffer_copy(urt_context* ctx, urt_handle src, int src_first, urt_handle dst, int dst_first, int count);

/* Linear blend skinning on the GPU.  rest_vertices (stride 12), rest_normals (stride 12; 0 is allowed exactly when dst_normals == 0),
 * bone_indices (stride 16: int32[4] per vertex), bone_weights (stride 16: float[4] per vertex), bones (stride 48: urt_ObjectMotion's
 * a[12] — three columns of the linear part, then the translation — object space to object space; n_bones is the buffer's count).
 * rest_*, bone_indices, bone_weights and the destinations have one common count. */
typedef struct urt_SkinBuffers {
  urt_handle rest_vertices, rest_normals, bone_indices, bone_weights, bones;
} urt_SkinBuffers;   /* 40 bytes */
/* Skins elements first .. first+count-1 into the device mirrors of dst_vertices (and dst_normals, unless 0).  NORMATIVE arithmetic:
 * float32, one rounding per operation, no fma, evaluated as written.  For vertex i: P rest position, N rest normal, j[0..3] bone
 * indices, w[0..3] weights.  Term k is LIVE when w[k] != 0.0f (a NaN weight is live) and 0 <= j[k] < n_bones; a term that is not live
 * contributes +0.0f per component and its bone is not read, so an index out of range is never a fault and never an error.  Live term,
 * with a = bones[j[k]].a and r = 0, 1, 2:
 *     q.r = ((a[r]*P.x + a[3+r]*P.y) + a[6+r]*P.z) + a[9+r]        t_k.r = w[k]*q.r
 *     m.r = (a[r]*N.x + a[3+r]*N.y) + a[6+r]*N.z                    u_k.r = w[k]*m.r
 * dst_vertices[i].r = ((t_0.r + t_1.r) + t_2.r) + t_3.r; s.r is the same sum over the u_k and L2 = dot(s, s) of urt_math.h.  When L2 > 0
 * and finite, dst_normals[i] = normalize(s) of urt_math.h = s * (1.0f / f_sqrt(L2)); otherwise dst_normals[i] = s as it is.  Weights are
 * not normalised; non-finite inputs flow through the arithmetic.
 * The inputs get mirrors (above: only what a SetData changed travels — per frame, the bones); ONE kernel is enqueued on the context's
 * stream, nothing is synchronised and deferred frames stay deferred.  The destination range becomes stale and dirty as a whole, exactly
 * as with urt_buffer_set_data_device.
 * URT_ERR_INVALID_ARGUMENT: NULL in, a range outside the buffers, strides or counts that do not fit, a destination equal to an input or
 * to the other destination, dst_normals without rest_normals.  URT_ERR_INVALID_HANDLE: a required handle that is 0 or unknown.
 * count == 0 returns URT_OK after the checks.  On any error nothing is enqueued or marked. */
URT_API int urt_skin_vertices(urt_context* ctx, const urt_SkinBuffers* in, int first, int count, urt_handle dst_vertices,
                              urt_handle dst_normals);
/* Where a stride-12 buffer's elements first .. first+count-1 are, read on the device (a host that skins on the GPU still owes the
 * reference's _MeshBVH leaf boxes, RM:405-433): out6[0..2] the component-wise min and out6[3..5] the max over the elements whose three
 * components are all finite, *out_n (may be NULL) their number; with none, out6 = (+inf, +inf, +inf, -inf, -inf, -inf).  One reduction
 * and a small second pass, then the call synchronises (URT_ERR_WATCHDOG as urt_synchronize reports it).  Min and max are exact, so the
 * result does not depend on the order of the reduction; signed zeros compare as values.
 * Errors as urt_buffer_set_data_range, plus URT_ERR_INVALID_ARGUMENT for a stride other than 12 and for NULL out6. */
URT_API int urt_buffer_bounds(urt_context* ctx, urt_handle buffer, int first, int count, float out6[6], int* out_n);
/* out4: the stale element range (first, last; first > last when it is empty), the bytes of the device mirror (0: none), the downloads
 * of this buffer since its creation. */
URT_API int urt_debug_buffer_state(urt_context* ctx, urt_handle buffer, uint64_t out4[4]);

/* ---- normals on the device ---------------------------------------------------------------------------------------------------------
 * RayTraceMaster.ComputeNormals (RM:340-368) for positions that live in a buffer's device mirror: what urt_host_compute_normals computes
 * on the host, bit for bit, written into the device side of a normals buffer, where the in-place update picks it up (option
 * "refit_vertices").  The reference gives a vertex every index slot, across all meshes, whose vertex position equals its own (-0 == +0;
 * coordinates below 2^-50 also weld pairwise under EPSILON = 3 * float.Epsilon, which is not transitive), sums the un-normalised face
 * normals of those slots in ascending slot order (a triangle with two such slots counts twice) and normalises.
 * That weld relation depends on positions.  A NORMALS PLAN finds it once, on the host, from the buffers' contents at plan time, for
 * the served vertices first .. first+count-1 against ALL index slots of `indices` (a vertex of another mesh at the same position
 * contributes).  Its canonical form, which urt_debug_build_normals_plan returns:
 *   tris     the needed triangles — those that own at least one slot in the list of a served vertex — in ascending original triangle
 *            number, three vertex indices each: the plan's OWN copy, validated at creation and never re-read from `indices`
 *   entries  compact triangle ids (positions in tris), one per contributing slot, each list in ascending slot order; the lists are laid
 *            out in the order of the first served vertex that uses them, and vertices of one position share one list
 *   ranges   {start, length} into entries, one per served vertex (a vertex no slot names: length 0)
 * CONTRACT: in the served rows the result of urt_compute_normals equals urt_host_compute_normals of the buffers' current contents
 * WHENEVER THE CURRENT POSITIONS WELD AS THE PLAN-TIME POSITIONS DID.  The contract covers the vertices buffer only: a host that
 * changes `indices`, or whose deformation merges or splits coincident vertices, makes a new plan.  A plan that is stale in this sense
 * still reads only its own validated tris: it is never a fault.
 * NORMATIVE arithmetic: float32, one rounding per operation, no fma, evaluated as written.  Per needed triangle (a, b, c):
 *     e1 = b - a, e2 = c - a per component;  face = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x)
 * per served vertex, from s = (0, 0, 0) and over its entries sequentially in their order:  s = s + face per component; then
 *     mag = f_sqrt((s.x*s.x + s.y*s.y) + s.z*s.z);   n = mag > 1e-5f ? (s.x / mag, s.y / mag, s.z / mag) : (0, 0, 0)
 * with IEEE division and the correctly rounded f_sqrt of urt_math.h.  A NaN mag fails the comparison and gives zeros, a served vertex
 * with an empty list gets (0, 0, 0); non-finite positions flow through the arithmetic and are never a fault and never an error.  One
 * vertex's sum is never split, chunked or tree-reduced: the order is the specification.
 * There are no urt_group_* twins of the calls of this section (urt_group_context reaches a rank's context). */
typedef struct urt_NormalsPlanInfo {
  int32_t first, count, n_lists, n_triangles, n_entries, max_valence;
  uint64_t device_bytes;
} urt_NormalsPlanInfo;   /* 32 bytes */
/* Makes a plan from the HOST copies of `vertices` (stride 12) and `indices` (stride 4, a count that is a multiple of 3) as they are now:
 * an explicitly synchronising set-up call — a stale range is downloaded first (counted by urt_debug_buffer_state) — which uploads the
 * plan and returns its handle.  count == 0 is allowed and gives an empty plan.  URT_ERR_INVALID_HANDLE: a buffer handle that is 0 or
 * unknown; URT_ERR_INVALID_ARGUMENT: strides or an index count that do not fit, a range outside the vertices buffer, NULL out_plan;
 * URT_ERR_SCENE: an index outside the vertices buffer; URT_ERR_OUT_OF_MEMORY.  On any error nothing is allocated. */
URT_API int urt_normals_plan_create(urt_context* ctx, urt_handle vertices, urt_handle indices, int first, int count, urt_handle* out_plan);
URT_API int urt_normals_plan_info(urt_context* ctx, urt_handle plan, urt_NormalsPlanInfo* out);
/* Gives the plan's device memory back (urt_context_destroy does the same).  A plan stays releasable after urt_buffer_release of its buffers. */
URT_API int urt_normals_plan_release(urt_context* ctx, urt_handle plan);
/* Recomputes the normals of the plan's served vertices from the CURRENT contents of its vertices buffer into the device mirror of
 * dst_normals (both buffers get mirrors): two kernels are enqueued on the context's stream — the face normals of the needed triangles
 * into a grow-only scratch of 16 bytes per face held by the context, then one served vertex per lane — nothing is synchronised and
 * deferred frames stay deferred.  dst_normals[first .. first+count-1] becomes stale and dirty as a whole, exactly as with
 * urt_skin_vertices; rows outside the served range are not written.
 * Checked before anything is enqueued or marked: URT_ERR_INVALID_HANDLE for an unknown plan, a plan whose vertices buffer was released,
 * a dst_normals that is 0 or unknown; URT_ERR_INVALID_ARGUMENT for a dst_normals whose stride is not 12, whose count differs from the
 * vertices buffer's, or that is the vertices buffer itself.  An empty plan returns URT_OK after the checks. */
URT_API int urt_compute_normals(urt_context* ctx, urt_handle plan, urt_handle dst_normals);
/* Host only, no GPU: the canonical plan above, for tests and for hosts that want to inspect it.  ranges takes 2 * count words, entries
 * up to cap_entries words, tris up to 3 * cap_tris words; out_sizes = n_entries, n_triangles, max_valence.  Every output pointer may be
 * NULL (to ask for the sizes first); an array that is given and too small is URT_ERR_INVALID_ARGUMENT, as are bad counts, NULL inputs
 * and a range outside the vertices; URT_ERR_SCENE: an index outside the vertices (urt_host_last_error). */
URT_API int urt_debug_build_normals_plan(const float* vertices, int n_vertices, const int32_t* indices, int n_indices, int first, int count,
                                         int32_t* ranges, int32_t* entries, int cap_entries, int32_t* tris, int cap_tris,
                                         int32_t out_sizes[3]);

/* ---- blend shapes on the device -----------------------------------------------------------------------------------------------------
 * The first stage of a Unity SkinnedMeshRenderer: blend shapes (morph targets) — per-target vertex deltas, scaled by the target's weight
 * and added to the rest pose BEFORE the bones.  A MORPH PLAN holds the deltas of all targets of the served vertices first ..
 * first+count-1, laid out per vertex; urt_morph_vertices applies it to rest buffers under a weight table, into the device side of the
 * destinations (which may be _Vertices / _Normals themselves, or intermediates that urt_skin_vertices takes as its rest pose).
 * The plan's canonical form, which urt_debug_build_morph_plan returns:
 *   order    the permutation of the input delta numbers sorted by vertex ascending, then target ascending, then input position
 *            ascending: duplicates of one (vertex, target) pair are kept and all count; no delta is pruned, not even an all-zero one
 *   ranges   {start, length} into order, one per served vertex (a vertex no delta names: length 0)
 * NORMATIVE arithmetic: float32, one rounding per operation, no fma, evaluated as written.  For served vertex i, p = rest_vertices[i]
 * and n = rest_normals[i]; over its entries e sequentially in plan order, with w = weights[e.target]: the entry is LIVE when w != 0.0f
 * (a NaN weight is live); a live entry does, for r = 0, 1, 2,
 *     p.r = p.r + w * e.dp[r]        n.r = n.r + w * e.dn[r]
 * and an entry that is not live does nothing at all (-0.0f stays -0.0f, an infinite delta under weight 0 makes no NaN).  Then
 * dst_vertices[i] = p and dst_normals[i] = n; with URT_MORPH_NORMALIZE, L2 = dot(n, n) of urt_math.h and dst_normals[i] = normalize(n) of
 * urt_math.h when L2 > 0 and finite, else n as it is (the rule of urt_skin_vertices).  A vertex with no live entry gets its rest position
 * bit for bit.  One vertex's sum is never split or tree-reduced: the order is the specification.  Non-finite inputs flow through the
 * arithmetic and are never a fault and never an error.
 * There are no urt_group_* twins of the calls of this section (urt_group_context reaches a rank's context). */
typedef struct urt_MorphDelta {
  int32_t vertex;   /* element number in the vertex buffers (absolute, not relative to `first`) */
  int32_t target;   /* 0 .. n_targets-1 */
  float dp[3];      /* position delta at weight 1 */
  float dn[3];      /* normal delta at weight 1 */
} urt_MorphDelta;   /* 32 bytes */
typedef struct urt_MorphPlanInfo {
  int32_t first, count, n_targets, n_entries, max_valence, n_touched;   /* n_touched: served vertices with at least one entry */
  uint64_t device_bytes;
} urt_MorphPlanInfo;   /* 32 bytes */
enum { URT_MORPH_NORMALIZE = 1 };
/* Makes a plan for the served vertices first .. first+count-1 from n_deltas deltas of n_targets targets; `deltas` is copied before the
 * call returns.  The plan is independent of any buffer.  n_deltas == 0 and count == 0 are both legal.  URT_ERR_INVALID_ARGUMENT: NULL
 * deltas with n_deltas > 0, a negative n_deltas or count, a negative first, a served range beyond 2^31 - 1, n_targets outside 1..4096,
 * NULL out_plan; URT_ERR_SCENE: a vertex outside the served range, a target outside 0..n_targets-1; URT_ERR_OUT_OF_MEMORY.  On any
 * error nothing stays allocated. */
URT_API int urt_morph_plan_create(urt_context* ctx, const urt_MorphDelta* deltas, int n_deltas, int n_targets, int first, int count,
                                  urt_handle* out_plan);
URT_API int urt_morph_plan_info(urt_context* ctx, urt_handle plan, urt_MorphPlanInfo* out);
/* Gives the plan's device memory back (urt_context_destroy does the same). */
URT_API int urt_morph_plan_release(urt_context* ctx, urt_handle plan);
/* Morphs the plan's served vertices.  rest_vertices, dst_vertices: stride 12; rest_normals, dst_normals: stride 12, rest_normals may be
 * 0 exactly when dst_normals is 0 (then no normal is read or written); weights: stride 4 and a count equal to the plan's n_targets.  All
 * 12-byte buffers have one common count, which is >= first+count.  Every buffer gets a mirror, as with urt_skin_vertices; ONE kernel is
 * enqueued on the context's stream, nothing is synchronised and deferred frames stay deferred.  dst_*[first .. first+count-1] becomes
 * stale and dirty as a whole, exactly as with urt_skin_vertices; rows outside the served range are not written.
 * Checked before anything is enqueued or marked: URT_ERR_INVALID_HANDLE for an unknown plan and for a required handle that is 0 or
 * unknown; URT_ERR_INVALID_ARGUMENT for unknown flags, URT_MORPH_NORMALIZE without dst_normals, dst_normals without rest_normals, strides
 * or counts that do not fit, a destination equal to an input or to the other destination.  An empty plan (count == 0) returns URT_OK
 * after the checks. */
URT_API int urt_morph_vertices(urt_context* ctx, urt_handle plan, urt_handle rest_vertices, urt_handle rest_normals, urt_handle weights,
                               urt_handle dst_vertices, urt_handle dst_normals, int flags);
/* Host only, no GPU: the canonical plan above, for tests and for hosts that want to inspect it.  ranges takes 2 * count words, order
 * n_deltas words; out_sizes = n_entries, max_valence, n_touched.  Every output pointer may be NULL.  Errors as urt_morph_plan_create
 * (urt_host_last_error). */
URT_API int urt_debug_build_morph_plan(const urt_MorphDelta* deltas, int n_deltas, int n_targets, int first, int count, int32_t* ranges,
                                       int32_t* order, int32_t out_sizes[3]);

/* ---- the object-level BVH on the device ---------------------------------------------------------------------------------------------
 * The leaf boxes of _MeshObjects and _Spheres and the implicit heap over them (_MeshBVH / _SphereBVH, one leaf per object), computed from
 * and written into the DEVICE side of buffers: what urt_host_mesh_leaf_bounds(literal = 0), urt_host_sphere_leaf_bounds(literal = 0) and
 * urt_host_build_object_bvh compute on the host, value for value, for a host whose vertices live on the device (urt_skin_vertices,
 * urt_morph_vertices) or that does not want the host pass.
 * All three calls enqueue on the context's stream and synchronise nothing; deferred frames stay deferred and urt_counters does not change.
 * Every buffer named gets a device mirror at first use, as with urt_skin_vertices.  The destination's WHOLE element range becomes stale
 * and dirty, exactly as with urt_buffer_set_data_device: a destination that is bound as _MeshBVH / _SphereBVH is picked up by the next
 * preparation, which downloads it as it downloads every device-written small table.  Checked before anything is enqueued or marked:
 * URT_ERR_INVALID_HANDLE for a handle that is 0 or unknown; URT_ERR_INVALID_ARGUMENT for a NULL context, strides or counts that do not
 * fit and a destination that is also an input.  On any error nothing is enqueued or marked.
 * There are no urt_group_* twins of the calls of this section (urt_group_context reaches a rank's context). */
/* mesh_objects (stride 112), vertices (stride 12), indices (stride 4), dst_leaves (stride 28, the count of mesh_objects).  Leaf m is what
 * urt_host_mesh_leaf_bounds(..., literal = 0, ...) writes, read from the CURRENT device contents of `vertices`.  With M the matrix of
 * MeshObject m, per index slot i of [indices_offset, indices_offset + indices_count): p = vertices[indices[i]] and, for r = 0, 1, 2,
 *     w.r = ((M[r]*p.x + M[4+r]*p.y) + M[8+r]*p.z) + M[12+r]
 * in float32, one rounding per operation, no fma; vmin / vmax = the component-wise min / max of the w, index = m.  A MeshObject with
 * indices_count == 0 gets an all-zero box and index = m.
 * The per-mesh (offset, count) and the matrices come from `mesh_objects`; the ranges are validated on that buffer's host copy (a stale
 * one is downloaded first: the one case in which this call synchronises): offset < 0, count < 0 or offset + count beyond `indices` is
 * URT_ERR_SCENE.  Index VALUES are not validated: a slot whose index lies outside `vertices` is skipped, which is never a fault and never
 * an error.  A NaN coordinate takes no part in that component's min or max; a component with no contributing value gets (+inf, -inf);
 * signed zeros compare as values.
 * CONTRACT: equal to the host function, by value, whenever every index is in range and no transformed coordinate is NaN.
 * Two kernels: per-workgroup partial boxes (at most URT_MESH_LEAF_BLOCKS workgroups per MeshObject, 256 slots each per pass) into a
 * grow-only scratch held by the context, then one workgroup per MeshObject.  Zero MeshObjects: URT_OK after the checks. */
URT_API int urt_mesh_leaf_bounds_device(urt_context* ctx, urt_handle mesh_objects, urt_handle vertices, urt_handle indices,
                                        urt_handle dst_leaves);
#define URT_MESH_LEAF_BLOCKS 256
/* spheres (stride 56), dst_leaves (stride 28), equal counts.  Per component a = position - (-radius), b = position - radius,
 * vmin = min(a, b), vmax = max(a, b), index = i: urt_host_sphere_leaf_bounds(literal = 0), equal by value for all non-NaN inputs. */
URT_API int urt_sphere_leaf_bounds_device(urt_context* ctx, urt_handle spheres, urt_handle dst_leaves);
/* leaves and dst_nodes have stride 28; with n = the count of leaves, dst_nodes has the count urt_host_object_bvh_length(n).
 * n > URT_OBJECT_BVH_DEVICE_MAX is URT_ERR_INVALID_ARGUMENT (the kernel is one workgroup, the object walk's stack is 32 deep and the
 * reference's scenes hold 6 to 21 objects): such a heap is built with urt_host_build_object_bvh.
 * The result is what urt_host_build_object_bvh(leaves, n, ...) writes, read from the current device contents of `leaves`.  NORMATIVE:
 *   - the heap is implicit, children of node i at 2i+1 and 2i+2; the root holds the range of all n leaves;
 *   - filler nodes are all zero with index = -1;
 *   - a one-object range copies its leaf record verbatim: box corners as given, inverted boxes included, and the leaf's own index field;
 *   - an interior node is the union over min(vmin, vmax) / max(vmin, vmax) of its leaves, with index = -1;
 *   - centres are 0.5f*vmin + 0.5f*vmax per component;
 *   - the axis: start with ax = 0; move to 1 if extent 1 is greater than extent 0; then move to 2 if extent 2 is greater than the extent
 *     of ax.  Extents are max - min of the range's centres;
 *   - the range is ordered by (centre[ax], leaf number); the left child takes the first (cnt + 1) / 2.
 * CONTRACT: integer fields equal bit for bit and floats equal by value, whenever every leaf coordinate is finite.  With non-finite
 * coordinates the call never faults and the heap stays well formed — every leaf appears exactly once — the device ordering keys by a
 * total order in which -0 = +0 and every NaN ranks above +inf; equality with the host is not promised there (the host's std::sort has
 * no defined answer for that input). */
URT_API int urt_build_object_bvh_device(urt_context* ctx, urt_handle leaves, urt_handle dst_nodes);
#define URT_OBJECT_BVH_DEVICE_MAX 1024

/* ---- RenderTexture / Texture (RGBA32F = ARGBFloat, linear) -------------------------------- */
/* new RenderTexture(w, h, 0, ARGBFloat, Linear){enableRandomWrite}.Create()   RM:834-840 */
URT_API int urt_texture_create(urt_context* ctx, int width, int height, urt_handle* out_texture);
/* Same, over caller-owned device memory of width*height*16 bytes (e.g. a torch tensor that a
 * collective reads); the library never frees it. */
URT_API int urt_texture_create_external(urt_context* ctx, int width, int height, void* device_ptr,
                                        urt_handle* out_texture);
/* Upload / read back width*height*4 floats, row 0 = bottom.  (sky texture upload; readback stands
 * in for presenting _converged, RM:819.)  Both synchronise. */
URT_API int urt_texture_set_pixels(urt_context* ctx, urt_handle texture, const float* rgba);
URT_API int urt_texture_get_pixels(urt_context* ctx, urt_handle texture, float* rgba);
/* Pipelined readback for a host that LOOKS at every frame on the CPU (the reference presents on the GPU, RM:819; a host on another
 * device — or Unity's own `destination` behind the shim — needs the pixels in host memory).  urt_texture_get_pixels waits for the frame
 * and then for 33 MB over PCIe into pageable memory (2.2 ms at 1080p) before the next frame can start.  begin: submits the deferred
 * work, snapshots the image AS IT IS AT THIS POINT of the program order (a device copy on the render stream) and sends the snapshot to a
 * pinned host image on a copy stream of the library's own — it returns at once and later frames render while the snapshot travels;
 * end: waits for that one copy and hands out the pinned image (width x height x 4 floats, row 0 = bottom), valid until the third
 * urt_texture_read_begin after the one that made the ticket.  Up to three readbacks may be in flight.  A watchdog trip is reported by end. */
URT_API int urt_texture_read_begin(urt_context* ctx, urt_handle texture, uint64_t* out_ticket);
URT_API int urt_texture_read_end(urt_context* ctx, uint64_t ticket, const float** out_rgba);
/* The same readback in the FORMAT of the host's `destination` (RM:819 blits _converged into whatever the camera renders to): the image
 * is converted on the GPU (csrc/present.hip) and only the converted pixels cross the bus — 8.3 MB (RGBA8) or 16.6 MB (RGBA16F) per 1080p
 * frame instead of 33.2 MB.
 *   URT_FORMAT_RGBA32F     as urt_texture_read_begin
 *   URT_FORMAT_RGBA8_SRGB  bytes R, G, B, A per pixel: colour through the sRGB transfer function (the project renders in linear colour
 *                          space, ProjectSettings/ProjectSettings.asset:50, so a blit into an 8-bit back buffer encodes) — exactly the
 *                          bytes of urt_host_encode_srgb8 / urt_host_write_png; alpha as UNORM8
 *   URT_FORMAT_RGBA16F     four IEEE halfs per pixel, round to nearest even (a camera with allowHDR: ARGBHalf)
 * end_format: *out_pixels = the pinned host image (row 0 = bottom), *out_bytes (may be NULL) its size.  Tickets of converted images
 * must be ended with urt_texture_read_end_format. */
enum { URT_FORMAT_RGBA32F = 0, URT_FORMAT_RGBA8_SRGB = 1, URT_FORMAT_RGBA16F = 2 };
URT_API int urt_texture_read_begin_format(urt_context* ctx, urt_handle texture, int format, uint64_t* out_ticket);
URT_API int urt_texture_read_end_format(urt_context* ctx, uint64_t ticket, const void** out_pixels, size_t* out_bytes);
URT_API int urt_texture_get_info(urt_context* ctx, urt_handle texture, int* out_width, int* out_height,
                                 void** out_device_ptr);
/* texture.Release()                                                  RM:830-831 */
URT_API int urt_texture_release(urt_context* ctx, urt_handle texture);

/* ---- ComputeShader (RayTraceShader.compute; kernel index 0 = CSMain) ---------------------- */
/* shader.SetBuffer(0, name, buffer)                                  RM:255-259, names RM:787-794:
 *   _MeshObjects(112) _Vertices(12) _Indices(4) _Normals(12) _Spheres(56) _MeshBVH(28) _SphereBVH(28)
 * A name that was never bound counts as an empty buffer (RM:256 skips null; RS:375-379).
 * buffer == 0 unbinds. */
URT_API int urt_shader_set_buffer(urt_context* ctx, int kernel, const char* name, urt_handle buffer);
/* shader.SetTexture(0, "_SkyboxTexture" | "Result", tex)             RM:776, RM:803 */
URT_API int urt_shader_set_texture(urt_context* ctx, int kernel, const char* name, urt_handle texture);
/* shader.SetMatrix("_CameraToWorld" | "_CameraInverseProjection", m) RM:773-774 */
URT_API int urt_shader_set_matrix(urt_context* ctx, const char* name, const float* m16);
/* shader.SetVector("_PixelOffset", v)  (x,y used)                    RM:777 */
URT_API int urt_shader_set_vector(urt_context* ctx, const char* name, const float* v4);
/* shader.SetFloat("_Seed", v)                                        RM:778 */
URT_API int urt_shader_set_float(urt_context* ctx, const char* name, float value);
/* shader.SetInt("_numBounces" | "_numRays", v); "_MeshBVH_len" / "_SphereBVH_len" are accepted and
 * ignored (they are `static const` in the shader, RS:73-74).         RM:780-784
 * Names the shader does not declare are ignored, as Unity does. */
URT_API int urt_shader_set_int(urt_context* ctx, const char* name, int value);
/* shader.Dispatch(0, groupsX, groupsY, 1): one thread per pixel in 8x8 groups; threads outside the
 * Result texture write nothing.  Asynchronous, in order.            RM:806-810 -> RS:431-469 */
URT_API int urt_shader_dispatch(urt_context* ctx, int kernel, int groups_x, int groups_y, int groups_z);
/* Multi-GPU form: the same dispatch restricted to group rows first_group_row, +row_stride, ...
 * (8 pixel rows each).  Pixels keep their GLOBAL id.xy, so the union over ranks
 * r = 0..N-1 of dispatch_rows(r, N) is bit-identical to one full dispatch (RS:78,434). */
URT_API int urt_shader_dispatch_rows(urt_context* ctx, int kernel, int groups_x, int groups_y, int groups_z,
                                     int first_group_row, int row_stride);

/* ---- Graphics.Blit ------------------------------------------------------------------------ */
/* _additionMaterial.SetFloat("_Sample", sample); Graphics.Blit(src, dst, _additionMaterial):
 * dst = src * a + dst * (1 - a) with a = 1 / (sample + 1), all four channels   RM:817-818, AS:9,39-41 */
URT_API int urt_blit_add(urt_context* ctx, urt_handle src, urt_handle dst, float sample);
/* Graphics.Blit(src, dst): copy — the present of the accumulated frame      RM:819
 * While frames are deferred the copy is queued behind them (see "Frame batching" above). */
URT_API int urt_blit(urt_context* ctx, urt_handle src, urt_handle dst);
/* Strip helpers for the frame-end gather: copy the 8-row strips first_group_row, +row_stride, ... of
 * an image to/from a dense device buffer (strip-major).  out_bytes reports the packed size. */
URT_API int urt_texture_pack_rows(urt_context* ctx, urt_handle texture, int first_group_row, int row_stride,
                                  void* device_dst, uint64_t* out_bytes);
URT_API int urt_texture_unpack_rows(urt_context* ctx, urt_handle texture, int first_group_row, int row_stride,
                                    const void* device_src);
/* The same de-interleave issued on a CALLER-GIVEN stream (e.g. the communication stream the gather ran on), without touching
 * the context's own stream: the caller orders it (the image must not be in use by the context's queued work — a dedicated
 * gather target never is).  Lets rank 0 de-interleave frame i while its render stream is already on frame i+1. */
URT_API int urt_texture_unpack_rows_on(urt_context* ctx, urt_handle texture, int first_group_row, int row_stride,
                                       const void* device_src, void* hip_stream);
/* The RGB forms (12 B per pixel instead of 16) for the gather of a RUNNING MEAN: AdditionShader blends the alpha channel like the
 * colours and its source alpha is a = 1 / (_Sample + 1) itself (AS:39-41), so after sample n the alpha of `_converged` is the same
 * value in every pixel — w_0 = a_0 a_0, w_n = a_n a_n + w_{n-1} (1 - a_n) in float32 — and need not travel: the ranks pack three
 * channels and the root passes that value as `alpha` when it de-interleaves.  hip_stream NULL = the context's own stream (deferred
 * and ordered like urt_texture_unpack_rows), else a caller-ordered stream like urt_texture_unpack_rows_on. */
URT_API int urt_texture_pack_rows_rgb(urt_context* ctx, urt_handle texture, int first_group_row, int row_stride,
                                      void* device_dst, uint64_t* out_bytes);
URT_API int urt_texture_unpack_rows_rgb(urt_context* ctx, urt_handle texture, int first_group_row, int row_stride,
                                        const void* device_src, float alpha, void* hip_stream);

/* ---- ray queries -------------------------------------------------------------------------- */
/* Batched "what does this ray hit?" against the scene bound to kernel 0 (RS:364-383 Trace, outside a frame): picking, line of sight,
 * shadow / occlusion tests.  With t_max = +inf a closest-hit query returns exactly what the frame kernels' Trace returns for that ray —
 * distance, position and normal by the same expressions, the ground plane, the reference's object walk and its tie rules included.
 *  - t_max is exclusive: a hit counts only if 0 < t < t_max; NaN or t_max <= 0 is a miss.
 *  - flags URT_QUERY_CLOSEST: out = urt_RayHit[n]; URT_QUERY_ANY: out = int32_t[n], 1 if anything is hit with 0 < t < t_max (the walk
 *    stops at the first such hit).
 *  - the scene is the one bound at call time: a changed scene is prepared first (after the deferred frames that read the old one);
 *    otherwise deferred frames stay deferred.  Queries never change urt_counters (rays, launches, ...) or the frame batching.
 *  - n == 0: URT_OK, nothing is launched; n < 0, a NULL pointer with n > 0 or unknown flags: URT_ERR_INVALID_ARGUMENT.
 * urt_ray_query: host memory; returns when `out` is filled (a synchronising call: it reports URT_ERR_WATCHDOG like urt_synchronize).
 * urt_ray_query_device: device pointers (d_rays 16-byte aligned, d_out 16-byte aligned for urt_RayHit, 4-byte for int32); enqueued on
 * the context's stream, returns at once — the caller orders and synchronises it, as with urt_texture_unpack_rows_on. */
enum { URT_QUERY_CLOSEST = 0, URT_QUERY_ANY = 1 };
URT_API int urt_ray_query(urt_context* ctx, const urt_Ray* rays, int n, void* out, int flags);
URT_API int urt_ray_query_device(urt_context* ctx, const void* d_rays, int n, void* d_out, int flags);

/* ---- radiance queries --------------------------------------------------------------------- */
/* Batched "how much light arrives along this ray?": path-traced samples with the scene's own materials, emission and sky — the whole of
 * CSMain's per-pixel loop (RS:440-468) outside a frame.  Light probes, irradiance volumes and lightmap texels (rays), and extra samples
 * for chosen pixels of the bound camera, e.g. the ones urt_reproject left without history (pixels).  out = n RGBA32F texels.  All
 * arithmetic is the normative float32 of urt_math.h; Trace and Shade are the frame kernels' own.
 *  - URT_RADIANCE_RAYS: in = urt_PathRay[n].  Query i: seed = in[i].seed, avg = 0; for each of the `samples` samples: res = 0,
 *    energy = 1, (o, d) = (origin, direction), then up to `bounces` iterations of  h = Trace(o, d); if (!Shade(...)) break;  with
 *    rand() = rand_next(seed, px, py); then avg += res.  out[i] = (avg.x / (float)samples, avg.y / ..., avg.z / ..., 1.0f).  The seed
 *    carries over from one sample to the next, as between a pixel's rays (RS:444); no camera-ray draws are made.
 *  - URT_RADIANCE_PIXELS: in = urt_PathPixel[n].  out[i] = the texel a frame dispatched now with _numRays = samples and
 *    _numBounces = bounces would write to Result[y * width + x]: the uniforms bound at call time (_CameraToWorld,
 *    _CameraInverseProjection, _PixelOffset, _Seed), the size of the texture bound as Result; each sample draws its two jitter rand()
 *    values and runs CreateCameraRay (RS:142-153, 448-449).  With samples == _numRays and bounces == _numBounces the output equals the
 *    frame's pixel bit for bit.
 *  - samples 1..4096; bounces 0..64 (0: every output is (0, 0, 0, 1)); n == 0: URT_OK, nothing is launched.
 *  - scene, ordering and counters as urt_ray_query: a changed scene is prepared first (after the deferred frames that read the old one);
 *    otherwise deferred frames stay deferred — unless pending work writes the texture bound as _SkyboxTexture, which is then submitted
 *    first.  urt_counters and the frame batching are never changed.
 *  - errors, checked before anything is enqueued or written: URT_ERR_INVALID_ARGUMENT for n < 0, a NULL pointer with n > 0, unknown
 *    flags, samples or bounces out of range and (host form) a pixel outside 0..width-1 x 0..height-1; URT_ERR_UNBOUND (pixels mode) when
 *    no texture is bound as Result or a camera matrix was never set.  The device form cannot look at its pixels: one outside the range
 *    gets (0, 0, 0, 0) and is not traced.
 * urt_radiance_query: host memory; returns when `out_rgba` is filled (a synchronising call, as urt_ray_query).
 * urt_radiance_query_device: device pointers (rays and output 16-byte aligned, pixels 8-byte aligned); enqueued on the context's stream,
 * returns at once — the caller orders and synchronises it. */
enum { URT_RADIANCE_RAYS = 0, URT_RADIANCE_PIXELS = 1 };
URT_API int urt_radiance_query(urt_context* ctx, const void* in, int n, int samples, int bounces, float* out_rgba, int flags);
URT_API int urt_radiance_query_device(urt_context* ctx, const void* d_in, int n, int samples, int bounces, void* d_out_rgba, int flags);

/* ---- feature buffers ---------------------------------------------------------------------- */
/* Per-pixel first-hit feature buffers ("AOVs") of the bound camera: what each pixel's camera ray hits, for denoiser guides (albedo,
 * normal), compositing (depth) and whole-frame picking (ids).  Each handle is an existing texture (own or external) or 0 for "not
 * wanted"; all given targets have the same size, and that size is the pixel grid.  Pixel (x, y) is texel y * width + x, row 0 at the
 * bottom, where the frame kernels write Result.
 *  - the camera ray uses the scene bound to kernel 0 and the uniforms set at call time (_CameraToWorld, _CameraInverseProjection):
 *    URT_AOV_PIXEL_CENTER: u = ((float)x + 0.5f) / (float)width * 2.0f - 1.0f (v likewise), then CreateCameraRay (RS:142-153); no jitter.
 *    URT_AOV_FRAME_RAY: the first camera ray (sample 0) that a frame dispatched now would trace for the pixel (_Seed, _PixelOffset and the
 *    two rand() draws of RS:448-449).
 *  - the ray is traced with t_max = +inf: the result is exactly what urt_ray_query returns for it (and the frame kernels' Trace).
 *  - targets (RGBA32F; int fields are stored as their bits):
 *      hit     position.xyz, distance                                  miss: (0, 0, 0, +inf)
 *      normal  normal.xyz, kind as a float value (1 ground, 2 sphere, 3 triangle)   miss: (0, 0, 0, 0)
 *      albedo  min(1 - specular, albedo) (RS:390; ground (0.5, 0.3, 0.15)), smoothness   miss: the sky radiance Shade returns (RS:420-427), 0
 *      id      object (sphere / MeshObject index, else -1), primitive (index slot of RS:243, else -1), u | v   miss: (-1, -1, 0, 0)
 *  - like every call that could observe the images, it submits the deferred frames first; then a stale scene is prepared.  The kernel
 *    is enqueued on the context's stream and the call returns without synchronising.  urt_counters are not changed.
 *  - URT_ERR_INVALID_ARGUMENT: all four handles 0, a handle given twice, sizes differ, a target bound as _SkyboxTexture, unknown flags;
 *    URT_ERR_INVALID_HANDLE: an unknown handle; URT_ERR_UNBOUND: _CameraToWorld or _CameraInverseProjection never set.  On any error
 *    nothing is written. */
enum { URT_AOV_PIXEL_CENTER = 0, URT_AOV_FRAME_RAY = 1 };
URT_API int urt_render_aov(urt_context* ctx, urt_handle hit, urt_handle normal, urt_handle albedo, urt_handle id, int flags);

/* ---- denoising ---------------------------------------------------------------------------- */
/* Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over the colour of `src` (typically the accumulated image, RM:12 _converged),
 * guided by the `hit` and `normal` feature buffers of urt_render_aov and optionally by `albedo` (0 = no demodulation).  All five images
 * are existing RGBA32F textures (own or external) of one size.  Per pixel p: c_p = src.rgb, a_p = src.a, n_p = normal.xyz,
 * k_p = normal.w, z_p = hit.w, A_p = albedo.rgb.
 *  1. p passes through when k_p == 0, z_p is not finite or <= 0, a component of c_p or n_p is not finite, or a component of the float
 *     quotient c_p / d_p (rule 2) is not finite or exceeds 2^120 in magnitude: dst = src bit for bit, and p is never a tap of another
 *     pixel.  Every other pixel is a surface pixel.  (2^120: every pass output is a convex combination of values <= 2^120, weights >= 0
 *     of sum <= 1, and its float evaluation adds at most ~28 roundings, so no sum reaches FLT_MAX and no later pass sees inf.)
 *  2. demodulation: d_p = fmaxf(A_p, 1e-3f) per channel (a NaN channel gives 1e-3) with an albedo target, else 1; the filter runs on
 *     c_p / d_p.
 *  3. pass i = 0 .. iterations - 1, tap spacing s = 2^i: taps q = p + s (dx, dy), dx, dy in -2..2; taps outside the image and pass-through
 *     taps are skipped (no clamping, no mirroring).  h = {1/16, 1/4, 3/8, 1/4, 1/16};
 *       w_pq = h[dx] h[dy] exp(-(|c_p - c_q|^2 / (sigma_color 2^-i)^2 + |n_p - n_q|^2 / sigma_normal^2 + ((z_p - z_q) / (sigma_depth z_p))^2))
 *     where a term whose sigma is <= 0 is left out;  c'_p = sum w_pq c_q / sum w_pq  (the centre tap always counts).  c is the previous
 *     pass's output.
 *  4. dst.rgb = c_p d_p after the last pass, dst.a = a_p.
 * The kernels fold the constants so that each tap costs one exp2f.  Domain: per channel, |result - formula in float64| <= 1e-4 (1 +
 * |formula|) where |c_p / d_p| <= 2^60 and every positive sigma (sigma_color 2^-i for each pass i that runs) and z_p lie in
 * [2^-60, 2^60]: there the squares and the folded constants stay normal floats.  Outside that, for every input that rule 1 lets through,
 * every filtered value c'_p before rule 4 is finite and lies within [min, max] of the c_q / d_q of the surface pixels q it can reach
 * (|q - p| <= 2 (2^iterations - 1) in x and y), widened by 1e-5 of the largest magnitude among them; dst.rgb = c'_p d_p may overflow,
 * at its own pixel only.
 * params == NULL: the defaults below (chosen on 4-frame accumulations of the mixed test scene and C4, DESIGN.md "Denoising").
 *  - like urt_render_aov, it submits the deferred frames first (src is usually a deferred blit's destination), then enqueues the passes
 *    on the context's stream and returns without synchronising.  The scene is not read (not prepared); urt_counters are not changed.
 *  - dst == src is allowed (the last pass reads src only at its own pixel).
 *  - scratch: three float4 images of the size, held by the context and grown on demand (URT_ERR_OUT_OF_MEMORY when that fails).
 *  - URT_ERR_INVALID_ARGUMENT: dst equal to hit, normal or albedo, or bound as _SkyboxTexture; sizes differ; iterations outside 1..5; a
 *    NaN sigma.  URT_ERR_INVALID_HANDLE: src, dst, hit or normal 0 or unknown, albedo unknown.  On any error nothing is written and
 *    nothing is enqueued. */
typedef struct urt_DenoiseParams {   /* 16 bytes */
  int32_t iterations;   /* 1..5: passes with tap spacing s = 1, 2, 4, 8, 16 */
  float sigma_color;    /* colour edge stop, halved every pass; <= 0: no colour term */
  float sigma_normal;   /* normal edge stop; <= 0: no normal term */
  float sigma_depth;    /* relative-depth edge stop; <= 0: no depth term */
} urt_DenoiseParams;
#define URT_DENOISE_DEFAULT_ITERATIONS 5
#define URT_DENOISE_DEFAULT_SIGMA_COLOR 8.0f
#define URT_DENOISE_DEFAULT_SIGMA_NORMAL 0.5f
#define URT_DENOISE_DEFAULT_SIGMA_DEPTH 0.1f
URT_API int urt_denoise(urt_context* ctx, urt_handle src, urt_handle dst, urt_handle hit, urt_handle normal, urt_handle albedo,
                        const urt_DenoiseParams* params);

/* ---- temporal reprojection ---------------------------------------------------------------- */
/* Keeps the accumulated image across a camera move (the "temporal" stage of SVGF-style pipelines): urt_reproject carries the history
 * accumulated under the previous camera into the current view, using the pixel-centre feature buffers of urt_render_aov under both
 * cameras, and urt_blit_add_history blends new frames in with a per-pixel sample count instead of the single _Sample of urt_blit_add.
 * A COUNT TEXTURE is an RGBA32F texture whose .x holds the per-pixel sample count (a float, may be fractional); .yzw are written as 0
 * and are reserved.  All images of one call are existing RGBA32F textures (own or external) of one size W x H, row 0 at the bottom.
 *
 * Arithmetic (normative): float32 with one rounding per operation, no fma, evaluated left to right as written; division is IEEE.
 * bits(f) = the int32 pattern of f.  Per pixel p = (x, y): k = normal.w, z = hit.w, P = hit.xyz, n = normal.xyz, o = bits(id.x);
 * M = prev_world_to_clip, C = _CameraToWorld, I = _CameraInverseProjection (the current uniforms).
 *  1. class of p: surface when k != 0, z finite and > 0, P and n finite; sky when k == 0; anything else has no history.
 *  2. projection into the previous view:
 *       surface: c_r = ((M[r]*P.x + M[4+r]*P.y) + M[8+r]*P.z) + M[12+r], r = 0 (cx), 1 (cy), 3 (cw);
 *       sky: the current pixel-centre ray: u = ((float)x + 0.5f) / (float)W * 2.0f - 1.0f, v likewise from y and H;
 *            e_r = (I[r]*u + I[4+r]*v) + I[12+r] (r = 0..2); d_r = (C[r]*e0 + C[4+r]*e1) + C[8+r]*e2;
 *            c_r = (M[r]*d0 + M[4+r]*d1) + M[8+r]*d2 for r = 0, 1, 3 (the direction at infinity, w = 0);
 *     then qx = ((cx / cw + 1.0f) * 0.5f) * (float)W - 0.5f, qy likewise from cy and H.  No history unless cw > 0 and
 *     qx > -1 && qx < W && qy > -1 && qy < H (NaN fails every comparison).
 *  3. bilinear taps: fx = qx - floorf(qx), gx = 1.0f - fx (fy, gy likewise), x0 = (int)floorf(qx), y0 = (int)floorf(qy); taps in this
 *     order: (x0,y0) gx*gy, (x0+1,y0) fx*gy, (x0,y0+1) gx*fy, (x0+1,y0+1) fx*fy.  A tap q is valid when it is inside the image, its weight
 *     is > 0, prev_count[q].x is finite and > 0 and all four components of prev_color[q] are finite, and in addition
 *       sky p: prev_normal[q].w == 0;
 *       surface p: prev_normal[q].w == k, bits(prev_id[q].x) == o, prev_hit[q].w finite and > 0,
 *                  (n.x*m.x + n.y*m.y) + n.z*m.z >= normal_threshold with m = prev_normal[q].xyz, and
 *                  fabsf((n.x*(Q.x-P.x) + n.y*(Q.y-P.y)) + n.z*(Q.z-P.z)) <= plane_threshold * z with Q = prev_hit[q].xyz.
 *  4. sums over the valid taps in tap order from 0.0f: S = sum w, A = sum w*prev_color[q] (per component), N = sum w*prev_count[q].x.
 *     History exists when S >= 0.01f: color = A / S per component, count = N / S, and count = fminf(count, max_history) when
 *     max_history > 0.  Without history color = (0,0,0,0), count = 0.  The count texel is written as (count, 0, 0, 0).
 *  5. motion (when wanted): (qx - (float)x, qy - (float)y, S, 0) when step 2's window test passed, else (0,0,0,0).
 * urt_blit_add_history(src, dst, count, max_history): the AdditionShader blend of urt_blit_add with a per-pixel sample count.  n =
 *     count.x; s = 0 when n is not finite or < 0, else s = max_history > 0 ? fminf(n, max_history - 1.0f) : n; then as urt_blit_add
 *     a = 1.0f / (s + 1.0f), ia = 1.0f - a, dst.rgb = t.rgb*a + c.rgb*ia, dst.a = a*a + c.a*ia (t = src, c = dst); count = (s + 1, 0, 0, 0).
 *     With a uniform count n and max_history == 0 it is bit for bit urt_blit_add(src, dst, n).
 * Calls:
 *  - urt_reproject is an observer like urt_denoise: it submits the deferred frames first (prev_color is usually a deferred blend's
 *    destination), then enqueues one kernel on the context's stream and returns without synchronising.  The scene is not read (not
 *    prepared); urt_counters are not changed.  motion = 0: not written.
 *  - urt_blit_add_history is deferred like urt_blit_add when src is the pending batch's Result texture; runs of such blends of consecutive
 *    frames into one dst / count / max_history, and a present (urt_blit) of dst after them, are fused into one pass with the same per-pixel
 *    operations.  Every call that observes dst or count submits them first.
 *  - URT_ERR_INVALID_ARGUMENT: NULL images or params; nonzero flags; a NaN threshold; max_history NaN, negative or in (0, 1); sizes that
 *    differ; an output equal to an input or to another output; an output bound as _SkyboxTexture; for the blend: count equal to src or
 *    dst, or src == dst.  URT_ERR_INVALID_HANDLE: a required handle 0 or unknown (motion may be 0).  URT_ERR_UNBOUND (urt_reproject):
 *    _CameraToWorld or _CameraInverseProjection never set.  Every argument is checked first: on any error nothing is written and nothing
 *    is enqueued.
 * The defaults below were chosen with the quality test of tests/test_gpu_reproject.py (DESIGN.md "Temporal reprojection").
 * urt_reproject projects the CURRENT world position of a pixel's hit point: right for a camera move over a still scene.  For objects that
 * have moved since the history was accumulated, urt_reproject_objects (below) projects the point where it WAS. */
typedef struct urt_ReprojectParams {     /* 80 bytes */
  float prev_world_to_clip[16];  /* the PREVIOUS camera's projection * worldToCamera, Unity Matrix4x4 memory order (column-major), the
                                    order urt_shader_set_matrix takes.  A Unity host: _camera.projectionMatrix *
                                    _camera.worldToCameraMatrix, kept from the frame before the move (RM:774 uses projectionMatrix). */
  float max_history;             /* 0 = unlimited, else >= 1: reprojected counts are clamped to it */
  float normal_threshold;        /* a history tap needs dot(n_p, n_q) >= this */
  float plane_threshold;         /* a history tap needs |dot(n_p, Q - P)| <= this * z_p */
  int32_t flags;                 /* 0 (reserved) */
} urt_ReprojectParams;
#define URT_REPROJECT_DEFAULT_MAX_HISTORY 64.0f
#define URT_REPROJECT_DEFAULT_NORMAL_THRESHOLD 0.9f
#define URT_REPROJECT_DEFAULT_PLANE_THRESHOLD 0.02f

typedef struct urt_ReprojectImages {     /* 11 handles, 88 bytes */
  urt_handle prev_color, prev_count;               /* the history as accumulated under the previous camera */
  urt_handle prev_hit, prev_normal, prev_id;       /* urt_render_aov(URT_AOV_PIXEL_CENTER) under the previous camera */
  urt_handle hit, normal, id;                      /* urt_render_aov(URT_AOV_PIXEL_CENTER) under the current camera */
  urt_handle color, count;                         /* out: the reprojected history */
  urt_handle motion;                               /* out, optional (0 = not wanted) */
} urt_ReprojectImages;

URT_API int urt_reproject(urt_context* ctx, const urt_ReprojectImages* images, const urt_ReprojectParams* params);
URT_API int urt_blit_add_history(urt_context* ctx, urt_handle src, urt_handle dst, urt_handle count, float max_history);

/* Per-object motion: urt_reproject for a scene whose MeshObjects and spheres have moved between the previous and the current feature
 * buffers (a refit, csrc/refit.hip).  A motion table is an ordinary buffer of urt_buffer_create with stride 48 whose entry i is the
 * urt_ObjectMotion (urt_types.h) of MeshObject i (mesh_motion) or of sphere i (sphere_motion): the affine map a[12] that takes a point of
 * the object in the CURRENT world to where it was in the PREVIOUS world.  A host fills the tables as it fills _MeshObjects;
 * urt_host_mesh_motion / urt_host_sphere_motion (below) compute the entries from the previous and the current object lists.  Motions
 * are meant to be rigid, optionally with uniform scale (normals are carried by the linear part, not by its inverse transpose).
 *
 * Arithmetic (normative), as urt_reproject's; only what differs:
 *  - moved pixel: a surface pixel with k == 3 (triangle) looks up mesh_motion[o], with k == 2 (sphere) sphere_motion[o], o = bits(id.x).
 *    The ground plane (k == 1), any other kind and the sky never move.  The pixel is MOVED when its table is given (handle != 0) and the
 *    twelve floats of its entry are not bit for bit the identity (1,0,0, 0,1,0, 0,0,1, 0,0,0).  A pixel that is not moved follows
 *    urt_reproject's steps exactly, operation for operation.  o outside 0 .. count-1 of a given table (count: the buffer's): the pixel
 *    has no history, as a pixel of no class in step 1 (colour, count and motion are 0).
 *  - position: P'.r = ((a[r]*P.x + a[3+r]*P.y) + a[6+r]*P.z) + a[9+r], r = 0..2.  A moved pixel uses P' in place of P in step 2.
 *  - normal: n'.r = (a[r]*n.x + a[3+r]*n.y) + a[6+r]*n.z, L = f_sqrt((n'.x*n'.x + n'.y*n'.y) + n'.z*n'.z) (f_sqrt of urt_math.h,
 *    correctly rounded on both sides).  L keeps the tests below free of the motion's scale without a division.
 *    A moved pixel has no history (as above: colour, count and motion are 0) unless P' is finite, L > 0 and L is finite.
 *  - tap tests of a moved pixel, evaluated in the previous frame: kind, id, prev_hit.w, count and colour as in step 3, and
 *      (n'.x*m.x + n'.y*m.y) + n'.z*m.z >= normal_threshold * L,
 *      fabsf((n'.x*(Q.x-P'.x) + n'.y*(Q.y-P'.y)) + n'.z*(Q.z-P'.z)) <= (plane_threshold * z) * L      (z = hit.w, the current distance).
 *  - count: after max_history's clamp, count = fminf(count, moved_max_history) on a moved pixel when moved_max_history > 0.  (Lighting
 *    on a moved object is stale - reflections, the sky it faces - so a host wants it to re-converge faster than the rest.)
 *  - motion image: unchanged in form, (qx - x, qy - y, S, 0); with P' it holds true screen-space motion vectors.
 * With motion == NULL, with both handles 0, or with tables that hold only identity entries, the three outputs equal urt_reproject's bit
 * for bit.  Calls and errors as urt_reproject (an observer: deferred frames submitted first, the tables uploaded and one kernel enqueued
 * on the context's stream, no synchronisation; the scene is not prepared, urt_counters are not changed; every argument is checked first).
 * motion == NULL is allowed and means both handles 0 and moved_max_history 0.  URT_ERR_INVALID_HANDLE: a table handle that is not 0 and
 * unknown.  URT_ERR_INVALID_ARGUMENT: a table whose stride is not 48; nonzero flags; moved_max_history NaN, negative or in (0, 1).
 * What remains untracked: shadows and reflections CAST BY a moved object onto other surfaces (those pixels keep their history and
 * converge to the new lighting at the rate max_history allows). */
typedef struct urt_ReprojectMotion {     /* 24 bytes */
  urt_handle mesh_motion;        /* buffer of urt_ObjectMotion (stride 48), entry i = MeshObject i; 0 = no mesh has moved */
  urt_handle sphere_motion;      /* the same for spheres; 0 = no sphere has moved */
  float moved_max_history;       /* 0 = none, else >= 1: extra clamp of the reprojected count on moved-object pixels */
  int32_t flags;                 /* 0 (reserved) */
} urt_ReprojectMotion;

URT_API int urt_reproject_objects(urt_context* ctx, const urt_ReprojectImages* images, const urt_ReprojectParams* params,
                                  const urt_ReprojectMotion* motion);

/* Per-vertex motion: urt_reproject_objects for a scene in which MeshObjects have also changed SHAPE between the previous and the current
 * feature buffers (a deformation: skinning, cloth, blend shapes; csrc/refit.hip refits such a mesh in place).  The topology is the same
 * then and now (the contract of option "refit_vertices"), and the id feature buffer names, per pixel, the MeshObject, the triangle's
 * first index slot and the barycentrics of the hit, so the point a pixel shows now is found at the position it HAD by interpolating the
 * previous vertex positions of the same triangle.  prev_vertices is usually a snapshot of _Vertices taken with urt_buffer_copy before
 * the deformation; prev_mesh_objects is _MeshObjects as it was then, so an object that deforms and moves in one step needs no entry in
 * mesh_motion.
 *
 * Arithmetic (normative), as urt_reproject_objects'; only what differs:
 *  - deformed pixel: a surface pixel is DEFORMED when k == 3 (triangle), deform is given, o = bits(id.x) lies in 0 .. n-1 with n the
 *    common count of deformed and prev_mesh_objects, and deformed[o] != 0.  With deform given, a triangle pixel whose o lies outside
 *    0 .. n-1 has no history (colour, count and motion are 0).  A deformed pixel does not read its mesh_motion entry.  Every pixel that
 *    is not deformed follows urt_reproject_objects operation for operation.
 *  - triangle: i = bits(id.y), u = id.z, v = id.w.  No history unless 0 <= i <= n_indices - 3 and each j_r = indices[i + r], r = 0, 1, 2,
 *    lies in 0 .. n_prev_vertices - 1 (the counts are the buffers').  An index out of range is never a fault and never an error.
 *  - previous position: with A_r = prev_vertices[j_r] and m = the 16 floats of prev_mesh_objects[o] (localToWorldMatrix, column-major):
 *      V_r.c = ((m[c]*A_r.x + m[4+c]*A_r.y) + m[8+c]*A_r.z) + m[12+c], c = 0..2;  w = (1.0f - u) - v;
 *      P'.c = (V_0.c*w + V_1.c*u) + V_2.c*v.
 *  - previous face normal: e1 = V_1 - V_0, e2 = V_2 - V_0 (per component),
 *      g = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x), L = f_sqrt((g.x*g.x + g.y*g.y) + g.z*g.z).
 *    No history unless P' is finite, L > 0 and L is finite (a NaN barycentric, a previous triangle without area).
 *  - from here on the pixel is a MOVED pixel of urt_reproject_objects with P' and n' = g: step 2 projects P'; the tap tests on kind,
 *    object id, prev_hit.w, count and colour are the same; the plane test is
 *      fabsf((g.x*(Q.x-P'.x) + g.y*(Q.y-P'.y)) + g.z*(Q.z-P'.z)) <= (plane_threshold * z) * L,
 *    the normal test is (g.x*m.x + g.y*m.y) + g.z*m.z >= deform->normal_threshold * L (m = prev_normal[q].xyz); moved_max_history clamps
 *    the count as on a moved pixel; the motion image is unchanged in form and holds the true screen-space motion of the deforming surface.
 *    The normal test has a threshold of its own because g is a FACE normal while the tap's m is an interpolated shading normal: on a
 *    coarse mesh the two differ by a few tens of degrees, and params->normal_threshold (0.9) would refuse sound taps.
 * With deform == NULL, or with every element of deformed zero (and every triangle pixel's o inside 0 .. n-1), the three outputs equal
 * urt_reproject_objects' bit for bit.  Calls and errors as urt_reproject_objects (an observer: deferred frames submitted first, one
 * kernel enqueued on the context's stream, no synchronisation; the scene is not prepared, urt_counters are not changed; every argument is
 * checked first and on any error nothing is written or enqueued).  The four buffers are read through their device mirrors (the
 * section "the device side of a ComputeBuffer"): no download is made, and urt_debug_buffer_state shows none.
 * URT_ERR_INVALID_HANDLE: a handle of a given deform that is 0 or unknown.  URT_ERR_INVALID_ARGUMENT: a stride other than 12 / 4 / 112 /
 * 4; an indices count that is not a multiple of 3; counts of deformed and prev_mesh_objects that differ; nonzero flags; a NaN threshold.
 * The default below was chosen with the quality test of tests/test_gpu_reproject_deform.py (DESIGN.md "Per-vertex motion").
 * What remains untracked: shadows and reflections cast by a deforming mesh onto other surfaces, as for moved objects; the shading
 * normals of the previous frame are not consulted. */
typedef struct urt_ReprojectDeform {     /* 40 bytes */
  urt_handle prev_vertices;      /* stride 12: object-space positions as _Vertices held them when the history was accumulated */
  urt_handle indices;            /* stride 4: the buffer bound as _Indices (same topology then and now) */
  urt_handle prev_mesh_objects;  /* stride 112: _MeshObjects as it was then; only localToWorldMatrix (@0, 16 floats) is read */
  urt_handle deformed;           /* stride 4: one int32 per MeshObject, nonzero = its triangle pixels take the per-vertex path */
  float normal_threshold;        /* per-vertex path only: a history tap needs dot(g, n_q) >= this * |g|; NaN is an error */
  int32_t flags;                 /* 0 (reserved) */
} urt_ReprojectDeform;
#define URT_REPROJECT_DEFAULT_DEFORM_NORMAL_THRESHOLD 0.3f

URT_API int urt_reproject_deformed(urt_context* ctx, const urt_ReprojectImages* images, const urt_ReprojectParams* params,
                                   const urt_ReprojectMotion* motion /* may be NULL */, const urt_ReprojectDeform* deform /* may be NULL */);

/* ---- resampling --------------------------------------------------------------------------- */
/* The step after urt_reproject, kept on the GPU: find the pixels whose history is short (urt_select_pixels), trace fresh samples for them
 * (urt_radiance_query_device, URT_RADIANCE_PIXELS, over the list) and blend the samples back into the accumulated image and its count
 * texture (urt_blend_samples); urt_resample_below is the three in one call for hosts without device memory of their own.  With
 * below == 1 the pixels a reprojection left without history are resampled; with below > 1 the same calls are a simple adaptive sampler
 * that gives more samples to pixels whose history is short.  Count textures and image layout as in "temporal reprojection" above.
 *
 * urt_select_pixels(count, below, d_pixels, capacity, out_n): ordered stream compaction of a count texture (W x H) into a pixel list.
 *  - pixel (x, y) is selected when !(count[y * W + x].x >= below): NaN, negative and -inf counts are selected, +inf is not.
 *  - the selected pixels are written as urt_PathPixel {x, y} in ascending texel index y * W + x: a dense list that starts at d_pixels[0]
 *    and holds at most `capacity` entries; entries from `capacity` on are not touched.  The same texture and `below` give the same list.
 *  - *out_n = the total number selected, which may exceed capacity.  capacity == 0 with d_pixels == NULL only counts.
 *  - the call observes `count`: like urt_reproject it submits the deferred frames first; then it enqueues its kernels on the context's
 *    stream and SYNCHRONISES to return *out_n (it reports URT_ERR_WATCHDOG as urt_synchronize does).  The scene is not read (not
 *    prepared); urt_counters and the frame batching are not changed.
 *  - d_pixels: device memory, 8-byte aligned.  W * H <= 2^31 - 1.
 *  - errors, checked before anything is enqueued or written: URT_ERR_INVALID_ARGUMENT for a NaN `below`, capacity < 0, d_pixels == NULL
 *    with capacity > 0, d_pixels not 8-byte aligned, out_n == NULL, a texture of more than 2^31 - 1 texels; URT_ERR_INVALID_HANDLE for
 *    `count` 0 or unknown.
 *
 * urt_blend_samples(d_pixels, d_samples, n, weight, dst, count, max_history): for i = 0 .. n-1 with (x, y) = d_pixels[i] inside dst — an
 * entry whose pixel lies outside is skipped, nothing is written for it —, t = d_samples[i] (RGBA32F), c = the dst texel and N = the .x of
 * the count texel at (x, y); arithmetic as stated in "temporal reprojection": float32, one rounding per operation, no fma:
 *     s  = 0 when N is not finite or < 0, else max_history > 0 ? fminf(N, fmaxf(max_history - weight, 0.0f)) : N
 *     a  = weight / (s + weight);  ia = 1.0f - a
 *     dst.rgb = t.rgb*a + c.rgb*ia;  dst.a = a*a + c.a*ia;  count = (s + weight, 0, 0, 0)
 *  - with weight == 1.0f this is urt_blit_add_history operation for operation: blending every pixel of an image with weight 1 gives the
 *    dst and count that urt_blit_add_history(src, dst, count, max_history) gives, bit for bit.
 *  - weight: the number of frame-equivalents the sample stands for (a sample of k times the frame's _numRays: k).
 *  - the pixels of a list must be distinct, as urt_select_pixels makes them.  For a duplicated pixel one of its entries wins; which one
 *    is unspecified.  Nothing else is affected.
 *  - the call writes dst and count: it submits the deferred frames first, then enqueues one kernel on the context's stream and returns
 *    without synchronising.  n == 0: URT_OK (after the checks), nothing is launched.  urt_counters are not changed.
 *  - d_pixels: device memory, 8-byte aligned; d_samples: device memory, 16-byte aligned.
 *  - errors, checked before anything is enqueued or written: URT_ERR_INVALID_ARGUMENT for n < 0, a NULL or misaligned pointer with n > 0,
 *    a weight that is not finite or <= 0, max_history NaN, negative or in (0, 1), dst == count, sizes that differ, dst or count bound as
 *    _SkyboxTexture; URT_ERR_INVALID_HANDLE for dst or count 0 or unknown.
 *
 * urt_resample_below(dst, count, below, samples, bounces, weight, max_history, out_n): urt_select_pixels(count, below), then
 * urt_radiance_query_device(URT_RADIANCE_PIXELS, samples, bounces) over the list, then urt_blend_samples(weight, dst, count, max_history).
 *  - dst, count and *out_n are bit for bit what the three separate calls produce.  The uniforms, _Seed included, are those bound at call
 *    time.
 *  - the pixel list and the samples live in scratch held by the context, grown on demand to what the SELECTED count needs (8 + 16 bytes
 *    per selected pixel, plus one word per 2048 texels): not image-sized.  URT_ERR_OUT_OF_MEMORY when that fails.
 *  - *out_n (out_n may be NULL) = the number of pixels resampled; when it is 0 nothing more is launched.
 *  - the call synchronises once, for the selected count; the trace and the blend are only enqueued.  urt_counters and the frame batching
 *    are not changed; a changed scene is prepared as urt_radiance_query_device does.
 *  - errors, checked before anything is enqueued or written: those of urt_blend_samples for weight, max_history, dst and count; a NaN
 *    `below`, samples outside 1..4096 or bounces outside 0..64 (as urt_radiance_query): URT_ERR_INVALID_ARGUMENT; URT_ERR_UNBOUND when no
 *    texture is bound as Result or a camera matrix was never set (the cases of pixels mode; here also when nothing is selected);
 *    URT_ERR_INVALID_ARGUMENT when dst and count do not have the size of the texture bound as Result. */
URT_API int urt_select_pixels(urt_context* ctx, urt_handle count, float below, void* d_pixels, int capacity, int* out_n);
URT_API int urt_blend_samples(urt_context* ctx, const void* d_pixels, const void* d_samples, int n, float weight, urt_handle dst,
                              urt_handle count, float max_history);
URT_API int urt_resample_below(urt_context* ctx, urt_handle dst, urt_handle count, float below, int samples, int bounces, float weight,
                               float max_history, int* out_n);

/* ---- guide-driven upsampling -------------------------------------------------------------- */
/* Trace at low resolution, present at full: the radiance is accumulated on a small pixel grid (w x h), the pixel-centre feature buffers
 * of urt_render_aov are rendered on both grids under one camera, and urt_upsample reconstructs the W x H image by a bilinear gather that
 * takes a low-resolution tap only where both grids saw the same surface.  A pixel no tap can serve gets the count 0, which is what
 * urt_resample_below fills with full-resolution paths.  The one call of this header that reads images of two sizes: the five low_*
 * images are RGBA32F textures of one size w x h, the others of one size W x H, row 0 at the bottom; any positive sizes (the low grid may
 * be the larger one, equal, or in a non-integer ratio).  Count textures as in "temporal reprojection" above.
 *
 * Arithmetic (normative), in the style of urt_reproject: float32 with one rounding per operation, no fma, evaluated left to right as
 * written; division is IEEE.  Per full-grid pixel p = (X, Y): k = normal.w, z = hit.w, P = hit.xyz, n = normal.xyz, o = bits(id.x).
 *  1. class of p: urt_reproject's step 1 (surface when k != 0, z finite and > 0, P and n finite; sky when k == 0); anything else has no
 *     result.
 *  2. position on the low grid: qx = (((float)X + 0.5f) * (float)w) / (float)W - 0.5f, qy likewise from Y, h and H.
 *  3. stage 1, bilinear: fx, gx, fy, gy, x0, y0, the tap order and the weights exactly as urt_reproject's step 3.  A tap q is valid when
 *     it is inside the w x h image, its weight is > 0, all four components of low_color[q] are finite, its count n_q is finite and > 0
 *     (n_q = low_count[q].x, or 1.0f without low_count), and in addition
 *       sky p: low_normal[q].w == 0;
 *       surface p: low_normal[q].w == k, bits(low_id[q].x) == o, low_hit[q].w finite and > 0,
 *                  (n.x*m.x + n.y*m.y) + n.z*m.z >= normal_threshold with m = low_normal[q].xyz, and
 *                  fabsf((n.x*(Q.x-P.x) + n.y*(Q.y-P.y)) + n.z*(Q.z-P.z)) <= plane_threshold * z with Q = low_hit[q].xyz.
 *     Sums over the valid taps in tap order from 0.0f: S = sum w, A = sum w*low_color[q] (per component), N = sum w*n_q.  A result
 *     exists when S >= 0.01f.
 *  4. stage 2, only with URT_UPSAMPLE_WIDE_FALLBACK and no stage-1 result: the sixteen texels (x0-1+i, y0-1+j), j = 0..3 outer,
 *     i = 0..3 inner, each with w = 1.0f; validity as in stage 1 without the weight test; the same sums, started again from 0.0f.  A
 *     result exists when S >= 1.0f.
 *  5. output: with a result color = A / S per component and count = ((N / S) * count_scale, 0, 0, 0); without one color = (0,0,0,0)
 *     and count = (0,0,0,0).  For a sky p with a result, with URT_UPSAMPLE_SKY_FROM_ALBEDO and an albedo image, color.rgb is replaced
 *     by albedo[p].rgb (urt_render_aov's miss value: the sky radiance, exact at full resolution); color.a stays.
 * Calls, as urt_reproject: an observer — it submits the deferred frames first (low_color is usually a deferred blend's destination), then
 * enqueues one kernel on the context's stream and returns without synchronising.  The scene is not read (not prepared); urt_counters
 * are not changed.  params == NULL means the defaults below.  Every argument is checked first: on any error nothing is written and
 * nothing is enqueued.
 *  - URT_ERR_INVALID_ARGUMENT: NULL images; unknown flags; a NaN threshold; count_scale not finite or <= 0; low images that are not all
 *    one size; full images that are not all one size; an output equal to an input or to the other output; an output bound as
 *    _SkyboxTexture.
 *  - URT_ERR_INVALID_HANDLE: a required handle that is 0 or unknown, or an optional handle (low_count, albedo, count) that is unknown.
 * Where the guides should look: a frame's samples of pixel (x, y) are centred on (x + 1, y + 1) (rand + _PixelOffset, RS:448-449), half
 * a pixel of the image's own grid from the pixel centre URT_AOV_PIXEL_CENTER looks through; half a low pixel is a whole full-grid pixel
 * at a ratio of 2.  A host that upsamples accumulated frames renders each set of guides with _CameraInverseProjection sheared by half a
 * pixel of that set's grid (translation column += column 0 / width + column 1 / height) and binds its own matrix again afterwards
 * (DESIGN.md §22); the call itself takes the guides it is given.
 * The thresholds start at the reprojection's own; the quality test of tests/test_gpu_upsample.py holds them. */
enum { URT_UPSAMPLE_WIDE_FALLBACK = 1, URT_UPSAMPLE_SKY_FROM_ALBEDO = 2 };
typedef struct urt_UpsampleParams {      /* 16 bytes */
  float normal_threshold;        /* a tap needs dot(n_p, n_q) >= this */
  float plane_threshold;         /* a tap needs |dot(n_p, Q - P)| <= this * z_p */
  float count_scale;             /* finite, > 0: out count = tap count * this (a host passes e.g. (w*h)/(W*H)) */
  int32_t flags;                 /* URT_UPSAMPLE_* */
} urt_UpsampleParams;
#define URT_UPSAMPLE_DEFAULT_NORMAL_THRESHOLD 0.9f
#define URT_UPSAMPLE_DEFAULT_PLANE_THRESHOLD 0.02f
#define URT_UPSAMPLE_DEFAULT_COUNT_SCALE 1.0f
#define URT_UPSAMPLE_DEFAULT_FLAGS URT_UPSAMPLE_WIDE_FALLBACK

typedef struct urt_UpsampleImages {      /* 11 handles, 88 bytes */
  urt_handle low_color, low_count;                 /* w x h: the traced image; low_count optional (0: every texel counts 1.0f) */
  urt_handle low_hit, low_normal, low_id;          /* w x h: urt_render_aov(URT_AOV_PIXEL_CENTER) on the low grid */
  urt_handle hit, normal, id;                      /* W x H: the same, on the full grid, same camera */
  urt_handle albedo;                               /* W x H, optional: read only for sky pixels (its miss value is the sky radiance) */
  urt_handle color, count;                         /* out, W x H; count optional */
} urt_UpsampleImages;

URT_API int urt_upsample(urt_context* ctx, const urt_UpsampleImages* images, const urt_UpsampleParams* params);

/* ---- auto-exposure and tone mapping ------------------------------------------------------- */
/* The last image-space stage ahead of an 8-bit present: the accumulated image is linear HDR radiance (HDR sky, emissive materials), and
 * the sRGB table of urt_texture_read_begin_format clamps whatever lies above 1.  urt_auto_exposure meters an RGBA32F image into a
 * caller-owned state in device memory; urt_tonemap scales an image by that exposure and maps it into [0, 1] with one of three
 * operators.  The result is an ordinary RGBA32F texture: urt_texture_read_begin_format(..., URT_FORMAT_RGBA8_SRGB) presents it as it
 * presents any other.  No new formats, no new options.
 *
 * Arithmetic (normative): float32 with one rounding per operation, no fma, evaluated left to right as written; division is IEEE; there
 * are no transcendentals.  bits(f) is the uint32 with the float's bit pattern, float_from_bits its inverse.
 *
 * urt_auto_exposure(ctx, src, count, params, d_state): src an RGBA32F texture, count an optional count texture of the same size (0: none;
 * "temporal reprojection" above), d_state caller-owned device memory, 16-byte aligned, holding a urt_ExposureState.  A zero-filled state
 * is a fresh one.
 *  1. per texel (r, g, b, .) of src: Y = (0.2126f*r + 0.7152f*g) + 0.0722f*b.  The texel is skipped, and counted in `skipped`, when Y
 *     is NaN, infinite or not > 0, or when a count texture is given and !(count.x > 0).  Otherwise it is counted in hist[k] with
 *     k = clamp((int)(bits(Y) >> 21) - 380, 0, 255): four bins per stop, Y == 1.0f in bin 128, 2^-32 .. 2^32.  counted = the sum of
 *     hist.  hist, counted and skipped are overwritten by every call.
 *  2. resolve, in unsigned 64-bit integers: T = counted, lo = T*low_permille/1000, hi = T*high_permille/1000 (floored).  The samples
 *     whose rank lies in [lo, hi), in ascending bin order, are kept: kept_k = the overlap of [prefix_k, prefix_k + hist[k]) with
 *     [lo, hi), prefix_k = hist[0] + .. + hist[k-1].  M = hi - lo.  With M == 0 exposure and target are left as they are.  Otherwise
 *       q = (sum k*kept_k * 256) / M,
 *       L = float_from_bits((380u << 21) + ((uint32_t)q << 13) + (1u << 20))     (the bin-centre luminance, piecewise-linear in bit space)
 *       target = fminf(fmaxf(key / L, min_exposure), max_exposure);
 *     when the previous exposure is not finite, is not > 0, or rate >= 1.0f: exposure = target; otherwise
 *     exposure = prev + (target - prev) * rate.  A host derives rate from its frame time (the library evaluates no exp).
 * urt_tonemap(ctx, src, dst, params, d_state): src and dst RGBA32F textures of one size; dst == src is allowed (in place).  d_state is
 * NULL or a urt_ExposureState in device memory, 16-byte aligned, read on the device (no synchronisation).
 *  1. s = state.exposure; e = s * params.exposure when s is finite and > 0; e = params.exposure when d_state is NULL or s is not.
 *  2. per colour channel c: x = c * e; if !(x > 0) x = 0, otherwise x = fminf(x, 65504.0f);
 *       URT_TONEMAP_LINEAR    y = x
 *       URT_TONEMAP_REINHARD  w2 = white*white, y = fminf((x * (1.0f + x / w2)) / (1.0f + x), 1.0f)
 *       URT_TONEMAP_ACES      y = fminf((x*(2.51f*x + 0.03f)) / (x*(2.43f*x + 0.59f) + 0.14f), 1.0f)
 *     alpha is copied bit for bit.
 * Calls, as urt_reproject: both are observers — they submit the deferred frames first (src is usually a deferred blend's destination),
 * then enqueue on the context's stream and return without synchronising; urt_auto_exposure zeroes the histogram itself.  The scene is
 * not read (not prepared); urt_counters are not changed.  params == NULL means the defaults below.  Every argument is checked first: on
 * any error nothing is written and nothing is enqueued.
 *  - urt_auto_exposure, URT_ERR_INVALID_ARGUMENT: d_state NULL or not 16-byte aligned; key, min_exposure or max_exposure not finite or
 *    <= 0; min_exposure > max_exposure; rate NaN or <= 0; permilles outside 0 <= low < high <= 1000; src and count of different sizes;
 *    more than 2^31 - 1 texels.
 *  - urt_tonemap, URT_ERR_INVALID_ARGUMENT: an unknown op; flags other than 0; exposure not finite or <= 0; white outside
 *    [0.01, 65504]; d_state not 16-byte aligned; src and dst of different sizes; dst bound as _SkyboxTexture.
 *  - URT_ERR_INVALID_HANDLE: src or dst 0 or unknown; a count that is not 0 and unknown. */
typedef struct urt_ExposureState {       /* 1040 bytes, in device memory; all zero = fresh */
  float exposure;                /* the exposure urt_tonemap multiplies by (0 or not finite: none yet) */
  float target;                  /* what the last metering asked for */
  uint32_t counted;              /* texels in hist */
  uint32_t skipped;              /* texels left out */
  uint32_t hist[256];            /* luminance histogram of the last call, four bins per stop */
} urt_ExposureState;
typedef struct urt_ExposureParams {      /* 24 bytes */
  float key;                     /* the metered luminance is exposed to this value (middle grey) */
  float min_exposure;            /* finite, > 0 */
  float max_exposure;            /* finite, >= min_exposure */
  float rate;                    /* > 0; >= 1 snaps to the target, below it the exposure moves this fraction of the way */
  int32_t low_permille;          /* the darkest low_permille / 1000 of the counted texels are left out of the mean ... */
  int32_t high_permille;         /* ... and those above high_permille / 1000; 0 <= low < high <= 1000 */
} urt_ExposureParams;
#define URT_EXPOSURE_DEFAULT_KEY 0.18f
#define URT_EXPOSURE_DEFAULT_MIN_EXPOSURE 0.015625f
#define URT_EXPOSURE_DEFAULT_MAX_EXPOSURE 64.0f
#define URT_EXPOSURE_DEFAULT_RATE 1.0f
#define URT_EXPOSURE_DEFAULT_LOW_PERMILLE 100
#define URT_EXPOSURE_DEFAULT_HIGH_PERMILLE 950

enum { URT_TONEMAP_LINEAR = 0, URT_TONEMAP_REINHARD = 1, URT_TONEMAP_ACES = 2 };
typedef struct urt_TonemapParams {       /* 16 bytes */
  float exposure;                /* finite, > 0: multiplies the state's exposure, or stands alone without one */
  float white;                   /* 0.01 .. 65504: the x that URT_TONEMAP_REINHARD maps to 1 */
  int32_t op;                    /* URT_TONEMAP_* */
  int32_t flags;                 /* 0 */
} urt_TonemapParams;
#define URT_TONEMAP_DEFAULT_EXPOSURE 1.0f
#define URT_TONEMAP_DEFAULT_WHITE 4.0f
#define URT_TONEMAP_DEFAULT_OP URT_TONEMAP_ACES
#define URT_TONEMAP_DEFAULT_FLAGS 0

URT_API int urt_auto_exposure(urt_context* ctx, urt_handle src, urt_handle count, const urt_ExposureParams* params, void* d_state);
URT_API int urt_tonemap(urt_context* ctx, urt_handle src, urt_handle dst, const urt_TonemapParams* params, const void* d_state);

/* ---- depth of field ----------------------------------------------------------------------- */
/* The camera of the trace kernels is a pinhole: everything is sharp.  urt_depth_of_field blurs a converged image by the circle of
 * confusion of a thin lens, in image space, from the depth urt_render_aov already provides: the `hit` target carries the camera ray's
 * hit distance in .w, +inf for the sky.  It costs nothing when it is not called, and a host pulls focus on a converged image without
 * tracing a ray.  A host orders the calls urt_auto_exposure, urt_depth_of_field, urt_bloom, urt_tonemap, formatted readback.  The result
 * is an ordinary RGBA32F texture.  No new formats, no new options.
 *
 * urt_depth_of_field(ctx, src, hit, dst, params): src, hit and dst RGBA32F textures of one size W x H, row 0 at the bottom; of hit only
 * .w is read.  dst is neither src nor hit: the gather reads neighbours, there is no in-place form.
 *
 * Arithmetic (normative): float32 with one rounding per operation, no fma, expressions evaluated as written; division is IEEE; f_sqrt
 * of urt_math.h is the correctly rounded square root; fminf / fmaxf are C's (of a NaN and a number, the number); there are no other
 * transcendentals.  With s = focus_distance, K = scale, Rmax = max_radius:
 *  1. Class of the pixel p.  z_p = hit[p].w, c_p = src[p].rgb.  p PASSES THROUGH when z_p is NaN or not > 0, or when a component of c_p
 *     is not finite or exceeds 2^100 in magnitude: dst[p] = src[p] bit for bit, and p is never a tap of another pixel.  Every other
 *     pixel is a LENS pixel; a distance of +inf (the sky) is one.  (2^100: a weight is at most 4 and a pixel has at most 1089 taps, so
 *     no sum below reaches FLT_MAX.)
 *  2. Blur radius, in pixels: a_p = fmaxf(fminf(fabsf(K * (1.0f - s / z_p)), Rmax), 0.5f).  A point in focus covers its own pixel,
 *     a = 0.5; for z = +inf, s / z = 0 and a = min(K, Rmax), clamped below by 0.5.  (Where s / z_p overflows and K is 0 the product is
 *     NaN and fminf returns Rmax: a distance below s / FLT_MAX is as far out of focus as a pixel gets.)
 *  3. Gather.  The taps of p are the lens pixels q = p + (dx, dy) inside the image, |dx| and |dy| <= 16, taken with dy ascending in the
 *     outer loop and dx ascending in the inner one.  For a tap
 *       d   = f_sqrt((float)(dx*dx + dy*dy))
 *       ae  = (z_q > z_p) ? fminf(a_q, a_p) : a_q
 *       cov = fminf(fmaxf((ae - d) + 0.5f, 0.0f), 1.0f)
 *       w   = cov / (ae * ae)
 *     (a point behind p never spreads onto p wider than p's own blur, so a sharp foreground stays sharp over a defocused background;
 *     near blur still bleeds over what lies behind it).  A tap whose cov is not > 0 is SKIPPED — it is not added as zero.  Over the
 *     remaining taps, in that order, from +0.0f: S = S + w and A.c = A.c + w * c_q.c per colour channel.  The own tap has cov = 1, so
 *     S > 0.
 *  4. Output: dst[p].c = A.c / S per colour channel; with URT_DOF_FLAG_COC dst[p].rgb = (a_p, a_p, a_p) instead, (0, 0, 0) at a
 *     pass-through pixel.  Alpha is src[p].a, bit for bit, in both cases.  One pixel's sum is never split or tree-reduced: the order is
 *     the specification.
 * How far an implementation looks.  A skipped tap contributes nothing at all, so the result does not depend on the taps visited as long
 * as every tap with cov > 0 is among them.  Rounding is monotonic, so d >= ae + 0.5 implies that cov is not > 0; ae <= a_q <= 16, so no
 * tap with |dx| or |dy| above 16 can count, and a tap q can count only for |dx|, |dy| <= d < a_q + 0.5.  An implementation may therefore
 * bound its loops by the largest a of the region the taps come from; the kernels do so per 16 x 16 tile (csrc/dof.hip).
 * Calls, as urt_bloom: an observer — it submits the deferred frames first, then enqueues on the context's stream and returns without
 * synchronising; dst counts as written by others.  The scene is not read (not prepared); urt_counters are not changed.  The
 * intermediates live in grow-only scratch of the context.  params == NULL means the defaults below.  Every argument is checked before
 * anything is enqueued or allocated for the call: on any error nothing is written.
 *  - URT_ERR_INVALID_ARGUMENT: ctx NULL; focus_distance not finite or <= 0; scale not finite or < 0; max_radius not in [0.5, 16] (NaN
 *    fails the test); unknown flag bits; textures of different sizes; dst == src or dst == hit; dst bound as _SkyboxTexture; textures
 *    taller than 1048560 pixels.
 *  - URT_ERR_INVALID_HANDLE: src, hit or dst 0 or unknown. */
#define URT_DOF_FLAG_COC 1              /* dst.rgb receives the pixel's blur radius a_p (pass-through pixels: 0, 0, 0) instead of the image */
#define URT_DOF_MAX_RADIUS 16.0f
typedef struct urt_DofParams {          /* 16 bytes */
  float focus_distance;   /* finite, > 0: the hit distance that is sharp, in scene units */
  float scale;            /* finite, >= 0: the blur radius in pixels of a point at infinity (K above) */
  float max_radius;       /* 0.5 .. URT_DOF_MAX_RADIUS: no pixel blurs wider than this */
  int32_t flags;          /* URT_DOF_FLAG_* */
} urt_DofParams;
#define URT_DOF_DEFAULT_FOCUS_DISTANCE 10.0f
#define URT_DOF_DEFAULT_SCALE 8.0f
#define URT_DOF_DEFAULT_MAX_RADIUS 8.0f
#define URT_DOF_DEFAULT_FLAGS 0
URT_API int urt_depth_of_field(urt_context* ctx, urt_handle src, urt_handle hit, urt_handle dst, const urt_DofParams* params);

/* ---- motion blur (urt_motion_blur) -------------------------------------------------------- */
/* A frame of the trace kernels is an instant: a host that moves something every frame and presents every frame gets a strobed image.
 * urt_motion_blur streaks a converged image along the screen-space motion its pixels had while the shutter was open, in image space,
 * from two images the library already produces: the `motion` image of urt_reproject / urt_reproject_objects / urt_reproject_deformed
 * ((qx - x, qy - y, S, 0): the displacement in pixels to where the pixel's point was, S > 0 where it is valid) and the `hit` target of
 * urt_render_aov (.w: the camera ray's hit distance, +inf for the sky).  It costs nothing when it is not called.  A host orders the
 * calls urt_auto_exposure, urt_depth_of_field, urt_motion_blur, urt_bloom, urt_tonemap, formatted readback.  The result is an ordinary
 * RGBA32F texture.  No new formats, no new options.
 *
 * urt_motion_blur(ctx, src, motion, hit, dst, params): src, motion, hit and dst RGBA32F textures of one size W x H, row 0 at the
 * bottom; of hit only .w is read, of motion .xyz.  dst is none of the three inputs: the gather reads neighbours, there is no in-place
 * form.  (The inputs may be one another.)
 *
 * Arithmetic (normative): float32 with one rounding per operation, no fma, expressions evaluated as written; division is IEEE; f_sqrt
 * of urt_math.h is the correctly rounded square root; fminf / fmaxf are C's (of a NaN and a number, the number); ceilf / floorf are
 * C's; there are no other transcendentals.  With h = shutter * 0.5f and R = max_radius:
 *  1. Class of the pixel p.  z_p = hit[p].w, c_p = src[p].rgb.  p PASSES THROUGH when z_p is NaN or not > 0, or when a component of c_p
 *     is not finite or exceeds 2^100 in magnitude: dst[p] = src[p] bit for bit, p is never a tap of another pixel and never decides a
 *     tile's velocity.  Every other pixel is a MOVING pixel, even at velocity 0; a distance of +inf (the sky) is one.
 *  2. Velocity of a moving pixel, in pixels, to either side of it.  t = motion[p]; when t.x and t.y are finite and t.z > 0,
 *     v = (h * t.x, h * t.y), else v = (0, 0).  l = f_sqrt(v.x*v.x + v.y*v.y); when l > R: s = R / l, v = (v.x * s, v.y * s).  Then
 *     per component v.c = fminf(fmaxf(v.c, -R), R): whatever the rounding, no tap offset exceeds 16.  Finally
 *     m_p = v.x*v.x + v.y*v.y and l_p = f_sqrt(m_p).  (A vector so long that the first sum overflows has l = inf, s = 0 and ends as
 *     v = 0: it is no motion a shutter could show.)  A pass-through pixel has m_p = -1.
 *  3. Tile velocity.  Tiles are 16 x 16 pixels, anchored at pixel (0, 0), ragged at the right and the top edge.  A tile's dominant pixel
 *     is the one with the largest m, among equal m the one with the lowest y * W + x; the tile carries its v and m.  A tile of
 *     pass-through pixels only has m = -1 and v = (+0, +0).  (An order-free maximum over a (value, index) key.)
 *  4. Neighbourhood velocity.  Of the tiles of a tile's 3 x 3 neighbourhood that lie inside the image, the one with the largest m,
 *     among equal m the first in the order dy ascending, then dx ascending: its v is n, its m is mn.
 *  5. Still tiles.  When mn is not >= 0.25f (nothing within reach moves half a pixel) every pixel of the tile gets dst[p] = src[p] bit
 *     for bit.
 *  6. Gather, everywhere else, for a moving pixel p.  M = (int)ceilf(fmaxf(fabsf(n.x), fabsf(n.y))), which is 1 .. 16.  For
 *     k = -M .. M ascending: dx = (int)floorf(((float)k * n.x) / (float)M + 0.5f), dy likewise from n.y.  A k whose (dx, dy) equals
 *     that of k - 1 is skipped (a repeated pixel of the line).  q = p + (dx, dy) is skipped when it lies outside the image or passes
 *     through.  Otherwise
 *       d   = f_sqrt((float)(dx*dx + dy*dy))
 *       ae  = (z_q < z_p) ? fmaxf(l_q, 0.5f) : fmaxf(l_p, 0.5f)
 *       cov = fminf(fmaxf(1.0f - d / ae, 0.0f), 1.0f)
 *       w   = cov / ae
 *     (what lies in front of p reaches it as far as ITS streak goes; what lies at or behind p's depth shows through as far as p's OWN
 *     streak makes p transparent: a still foreground stays sharp over a moving background, a moving foreground smears over a still
 *     background).  A tap whose cov is not > 0 is SKIPPED — it is not added as zero.  Over the remaining taps, in that order, from
 *     +0.0f: S = S + w and A.c = A.c + w * c_q.c per colour channel.  k = 0 is the own tap with cov = 1, so S > 0; w <= 2 and there
 *     are at most 33 taps, so with the 2^100 bound no sum reaches FLT_MAX.
 *  7. Output: dst[p].c = A.c / S per colour channel; alpha is src[p].a, bit for bit.  With URT_MOTION_BLUR_FLAG_VELOCITY
 *     dst[p].rgb = (n.x, n.y, l_p) instead, (n.x, n.y, 0) at a pass-through pixel, still tiles included (they are written, not
 *     copied); alpha as before.  One pixel's sum is never split or tree-reduced: the order is the specification.
 * Calls, as urt_depth_of_field: an observer — it submits the deferred frames first, then enqueues on the context's stream and returns
 * without synchronising; dst counts as written by others.  The scene is not read (not prepared); urt_counters are not changed.  The
 * intermediates live in grow-only scratch of the context.  params == NULL means the defaults below.  Every argument is checked before
 * anything is enqueued or allocated for the call: on any error nothing is written.
 *  - URT_ERR_INVALID_ARGUMENT: ctx NULL; shutter not finite or outside [0, 1]; max_radius not in [0.5, 16] (NaN fails the test);
 *    unknown flag bits; reserved != 0; textures of different sizes; dst == src, motion or hit; dst bound as _SkyboxTexture; textures
 *    taller than 1048560 pixels.
 *  - URT_ERR_INVALID_HANDLE: src, motion, hit or dst 0 or unknown. */
#define URT_MOTION_BLUR_FLAG_VELOCITY 1   /* dst.rgb = (n.x, n.y, l_p): the tile neighbourhood's dominant velocity and the pixel's own length */
#define URT_MOTION_BLUR_MAX_RADIUS 16.0f
typedef struct urt_MotionBlurParams {     /* 16 bytes */
  float shutter;      /* finite, 0 .. 1: the part of the frame interval the shutter is open; the streak is shutter * |motion| long */
  float max_radius;   /* 0.5 .. URT_MOTION_BLUR_MAX_RADIUS: no pixel streaks further than this to either side, in pixels */
  int32_t flags;      /* URT_MOTION_BLUR_FLAG_* */
  int32_t reserved;   /* 0 */
} urt_MotionBlurParams;
#define URT_MOTION_BLUR_DEFAULT_SHUTTER 0.5f
#define URT_MOTION_BLUR_DEFAULT_MAX_RADIUS 16.0f
URT_API int urt_motion_blur(urt_context* ctx, urt_handle src, urt_handle motion, urt_handle hit, urt_handle dst,
                            const urt_MotionBlurParams* params);

/* ---- bloom -------------------------------------------------------------------------------- */
/* The step between the exposure and the tone mapping: an emitter or the sun of an HDR sky lies many stops above white, and after
 * urt_tonemap it is a hard-edged white disc.  urt_bloom spreads what lies above a threshold over its surroundings, in linear radiance,
 * which is the only place where energy above 1.0 survives into an 8-bit frame.  A host orders the calls urt_auto_exposure, urt_bloom,
 * urt_tonemap, formatted readback.  The result is an ordinary RGBA32F texture.  No new formats, no new options.
 *
 * Arithmetic (normative): float32 with one rounding per operation, no fma, expressions evaluated as written; division is IEEE; there
 * are no transcendentals.  Row 0 is the bottom, as everywhere.
 *
 * urt_bloom(ctx, src, dst, params, d_state): src and dst RGBA32F textures of one size W x H; dst == src is allowed (in place).  d_state
 * is NULL or a urt_ExposureState in device memory, 16-byte aligned, read on the device (no synchronisation).
 *  Exposure.  s = state.exposure; e = s when d_state is given and 2^-60 <= s <= 2^60 (NaN fails that test), otherwise e = 1.
 *     t = threshold / e, cl = clamp / e, k = t * soft_knee: threshold and clamp are given in exposed units and applied to linear
 *     radiance.
 *  Level sizes.  w_0 = W, h_0 = H, w_l = (w_{l-1} + 1) >> 1, h_l likewise; L = min(levels, the first l at which w_l == h_l == 1), so
 *     L >= 1 always.
 *  Prefilter, per texel of src, colour channels only (level 0; it is never stored):
 *       c = (c > 0) ? fminf(c, 65504.0f) : 0                      (NaN, negatives, -0 -> 0; +inf -> 65504)
 *       m = fmaxf(fmaxf(r, g), b)
 *       q = fminf(fmaxf((m - t) + k, 0), 2*k);  q = (q*q) / (4*k + 1e-5f)
 *       g = fmaxf(q, m - t) / fmaxf(m, 1e-5f)
 *       g = g * fminf(1, cl / fmaxf(m, 1e-5f))
 *       p = c * g                                                 (per channel)
 *  Downsample, from level l-1 (a) to level l, for the coarse texel (x, y), with the fine columns x_j = clamp(2x - 1 + j, 0, w_{l-1} - 1),
 *     j = 0..3, and the fine rows y_j likewise:
 *       h(row) = (a[x_0] + a[x_3]) + 3*(a[x_1] + a[x_2])          for each of the four rows
 *       D_l    = ((h(y_0) + h(y_3)) + 3*(h(y_1) + h(y_2))) * 0.015625f
 *     (the binomial [1 3 3 1]^2 / 64, horizontal first).
 *  Upsample, from level l+1 (a) to the grid of level l, for the fine texel (x, y): n = x >> 1,
 *     f = clamp(n + ((x & 1) ? 1 : -1), 0, w_{l+1} - 1), and n_y, f_y likewise for the rows:
 *       h(row) = 3*a[n] + a[f]
 *       up     = (3*h(n_y) + h(f_y)) * 0.0625f
 *     U_L = D_L; U_l = D_l + (up(U_{l+1}) - D_l) * scatter for l = L-1 .. 1.
 *  Composite, with b = up(U_1) on the W x H grid: each colour channel of dst is src.c + b.c * intensity, with URT_BLOOM_FLAG_ONLY it is
 *     b.c * intensity.  Alpha is copied bit for bit.  Where a colour channel of src is NaN (without the flag), dst holds a NaN whose
 *     payload is unspecified; everything else is exact to the bit.
 * Calls, as urt_tonemap: an observer — it submits the deferred frames first, then enqueues on the context's stream and returns without
 * synchronising; dst counts as written by others.  The scene is not read (not prepared); urt_counters are not changed.  The pyramid
 * lives in grow-only scratch of the context.  params == NULL means the defaults below.  Every argument is checked before anything is
 * enqueued or allocated for the call: on any error nothing is written.
 *  - URT_ERR_INVALID_ARGUMENT: ctx NULL; threshold not in [0, 65504]; soft_knee or scatter not in [0, 1]; clamp not in (0, 65504];
 *    intensity not finite or < 0; levels not in 1..16; unknown flag bits; d_state not 16-byte aligned; src and dst of different sizes;
 *    dst bound as _SkyboxTexture; textures taller than 1048560 pixels.
 *  - URT_ERR_INVALID_HANDLE: src or dst 0 or unknown. */
#define URT_BLOOM_FLAG_ONLY 1            /* dst receives the bloom alone, not src + bloom */
typedef struct urt_BloomParams {         /* 28 bytes */
  float threshold;               /* 0 .. 65504, in exposed units: what lies below contributes nothing */
  float soft_knee;               /* 0 .. 1: the width of the quadratic knee below the threshold, as a fraction of it (0: a hard threshold) */
  float clamp;                   /* > 0 .. 65504, in exposed units: the brightest channel of a prefiltered texel is held to it */
  float scatter;                 /* 0 .. 1: how much of each coarser level reaches the next finer one (the width of the glow) */
  float intensity;               /* finite, >= 0: the weight of the bloom in dst */
  int32_t levels;                /* 1 .. 16: pyramid levels at most (the pyramid ends at 1 x 1) */
  int32_t flags;                 /* URT_BLOOM_FLAG_* */
} urt_BloomParams;
#define URT_BLOOM_DEFAULT_THRESHOLD 1.0f
#define URT_BLOOM_DEFAULT_SOFT_KNEE 0.5f
#define URT_BLOOM_DEFAULT_CLAMP 65504.0f
#define URT_BLOOM_DEFAULT_SCATTER 0.7f
#define URT_BLOOM_DEFAULT_INTENSITY 0.2f
#define URT_BLOOM_DEFAULT_LEVELS 6
#define URT_BLOOM_DEFAULT_FLAGS 0

URT_API int urt_bloom(urt_context* ctx, urt_handle src, urt_handle dst, const urt_BloomParams* params, const void* d_state);

/* ---- measurement -------------------------------------------------------------------------- */
typedef struct urt_counters {
  uint64_t rays;          /* Trace() invocations (RS:454) — the unit of the Mrays/s metric */
  uint64_t tlas_nodes;    /* object-level BVHNode fetches, 28 B each (RS:306, RS:341) */
  uint64_t blas_nodes;    /* triangle-BVH node visits, 64 B each */
  uint64_t tri_tests;     /* Moller-Trumbore evaluations, 48 B each (RS:199-234) */
  uint64_t sphere_tests;  /* IntersectSphere evaluations, 16 B each (RS:175-196) */
  uint64_t hit_tri;       /* closest hits shaded on a triangle: 48 B normals + 40 B material */
  uint64_t hit_sphere;    /* closest hits shaded on a sphere: 40 B material */
  uint64_t hit_ground;    /* closest hits on the y = 0 plane */
  uint64_t hit_sky;       /* paths ended on the sky: 4 x 16 B texels */
  uint64_t pixels;        /* pixels written (16 B each) */
  uint64_t dispatches;    /* urt_shader_dispatch* calls since reset */
  float trace_ms;         /* GPU time of the trace kernels of those dispatches (HIP events; needs "time_dispatch") */
  uint32_t watchdog_trips; /* waves that hit a persistent kernel's iteration cap (scaled with frames x rays x bounces of the launch): 0 unless
                              there is a bug; when not, the next urt_synchronize / urt_texture_get_pixels fails with URT_ERR_WATCHDOG */
  uint64_t launches;      /* trace-kernel launches those dispatches became (< dispatches when frames were batched) */
} urt_counters;
/* Options: "blas_builder" (-1 = auto, the default: 0 for scenes of fewer than 200,000 triangles, 3 from there on;
 *                          0 = binned-SAH triangle BVH built on host threads: best trees; 1 = LBVH built on the GPU
 *                          from the uploaded buffers — Morton sort + Karras hierarchy, csrc/lbvh.hip: milliseconds instead of tens
 *                          of milliseconds for scenes whose objects move; 2 = the same radix tree built top-down within a depth
 *                          budget ("lbvh_slack", default 6 levels beyond a median tree): the traversal stacks live in LDS and a
 *                          30-level Karras tree costs workgroups per CU — frames on tree 2 cost +6 ... +10 % against the SAH trees
 *                          instead of +10 ... +26 %, the build 1 ms more on a million triangles; 3 = BINNED SAH ON THE GPU — the host builder's
 *                          algorithm level by level with atomics: frames as on the host's trees, 15 ms instead of 80 for a million
 *                          triangles; same pixels whichever builder),
 *          "front_cull" (0/1, default 1: object-level cull — a MeshObject whose heap-leaf box the ray passes, leaves behind or meets
 *                        beyond the ground-plane hit, by a margin, is not intersected although the reference would (RS:294-326 keeps
 *                        testing every popped leaf once `tests` is set; such an object cannot hold the closest hit).  Only leaves whose
 *                        box the library has verified to contain the object's triangles; 0 = the reference's literal work),
 *          "overlap_launches" (0 off / 1 auto (default) / 2 always: launches of up to 8 frames — a host that submits every frame on its own,
 *                              urt_flush or a present per frame — alternate between two trace streams of the library's own and take their
 *                              Result slots round-robin, so that the next launch fills the wave slots the draining waves of the previous one
 *                              give back (C3, one frame per submission: 0.61 -> 0.50 ms per frame); blends, presents and readbacks stay on
 *                              the context's stream in program order.  Auto: not while a pipelined readback is in flight — a host that
 *                              waits for finished frames gets them later when two launches share the chip (+6 % C3, +21 % C2 with two
 *                              tickets in flight).  Only on the library's own stream),
 *          "frames_per_launch" (0 = auto: own stream -> up to 64 frames per launch (fewer if their Result slots exceed 8 GiB), caller's stream -> 1;
 *                               1 = every dispatch is its own launch; 2..64 = batch that many, also on a caller's stream),
 *          "count_stats" (0/1: per-dispatch traversal counters, slower build of the kernel),
 *          "time_dispatch" (0/1: bracket each dispatch with HIP events, read by urt_get_counters),
 *          "kernel_mode" (0 = one thread per pixel; 1 = one launch per bounce over compacted path queues;
 *                         2 = persistent waves with in-wave path regeneration;
 *                         3 = 2 + lanes scheduled by phase inside the wave, the default;
 *                         4 = 3 with a pool of 64 x pool_k paths per wave kept in LDS, experimental;
 *                         5 = 3 with the triangle-BVH phase as a service shared by the four waves of a workgroup (rays are
 *                             posted to a mailbox, any wave claims and walks them; "serve_refill" 1..64, "blas_min" up to 256):
 *                             measured alternative, slower than 3),
 *          "block_threads" (64 | 128 | 256: modes 0-2), "xcd_run" (0 = auto: 1..8 by launch size | >= 1: consecutive tiles a work-counter shard hands out as one run), "work_shards" (1 | 2 | ... | 64: work counters in use), "frame_group" (1..64: frames of a batched launch whose tile runs are interleaved; default 64 = all),
 *          "tile_order" (0 bottom-up | 1 top-down: a launch ends with the rows nearest the ground plane | -1 auto, the default: top-down for scenes without triangle meshes), "waves_per_cu" (0 = auto, 1..32), "refill_min" (1..64),
 *          mode 3: "blas_min" / "blas_exit" (0 = auto by scene | 1..64) / "shade_min" / "sky_min" (1..64): vote thresholds, "shade_split" (-1 auto | 0 | 1: surface hits and
 *                  sky misses as separate phases), "sched_block" (0 auto | 64 | 256),
 *                  "top_nodes" (0..256 triangle-BVH nodes kept in LDS; -1 auto, the default: 64, or twice the number of big MeshObjects when the object-level phase is the masked one), "top_front" (-1 auto | 0 | 1: where that top is
 *                  walked), "front_list" (-1 auto | 0 | 1 | 2: multi-mesh scenes determine the objects a ray must test first and work them off in voted
 *                  trips — auto / 1: by mask arithmetic over the heap when it has <= 31 nodes, else as a list when <= 12 MeshObjects; 2: always the list), "lds_tlas" (0/1: small object-level tables in LDS),
 *                  "front_fuse" (-1 auto, the default = on | 0 | 1: where the object-level phase is the plain one — one MeshObject, or "front_list" 0 — a new ray takes its
 *                  first object-level step in the trip that created it instead of waiting for a voted trip; same pixels, fewer scheduler trips),
 *                  "handout" (-1 auto, the default = 1 | 0 | 1: how the dead lanes of a wave get their next pixels — 0: every refill adds to the work counter of the
 *                  wave's shard, one device-scope atomic that the whole wave waits for; 1: the four waves of a workgroup share a reservation of up to 16 tiles
 *                  of a run in LDS, a refill is a compare-and-swap there and only the wave that drains it goes to the counter; same pixels in another order),
 *          mode 4: "pool_k" (1..4), "pool_refill", "pool_blas_min" (1..256), "pool_blas_exit", "pool_inloop",
 *                  "pool_other_min" (1..64),
 *          "blas_leaf_max" (1..8: triangles per BVH leaf, default 2 or the environment variable URT_BLAS_LEAF_MAX read when the
 *          library is loaded — a process-wide builder setting; rebuilds the BVH; changing it while another thread prepares a scene
 *          is not supported),
 *          "stack_pad" (0..96: test hook, unused extra entries per traversal stack -> the > 64 KiB LDS launch path),
 *          "radiance_persist" (-1 auto, the default | 0 | 1: urt_radiance_query on a resident grid whose lanes take the next query from a
 *                              work counter when theirs is finished, instead of one query per thread; same results),
 *          "qnodes" (0 off, the default | 1 on | -1 on unless some MeshObject spans fewer than 1024 grid cells: the traversal loop of the default
 *                    kernel reads 32-byte quantized copies of the triangle-BVH nodes — two vector loads per node step instead of four; conservative
 *                    boxes on one 16-bit grid over the whole forest, csrc/qnodes.hip; a forest too large for the grid's plane arithmetic (cell
 *                    > 2^43) keeps the float nodes, see urt_debug_read_scene_qnodes.  A measured alternative: same pixels, -1.3 % frame time on
 *                    single-mesh scenes, +1.3 % on C4 / C5: the loop waits on the latency of one dependent fetch per step, not on its width),
 *          "blas_cones" (-1 auto, the default = on | 0 off | 1 on: every child of a triangle-BVH node carries a cone that holds the normals of all
 *                        triangles below it — four signed bytes in the node's spare dwords, derived on the GPU after every build and refit,
 *                        csrc/cones.hip — and the traversal of the default kernel skips a child whose triangles the ray can only see from
 *                        behind: the reference's own back-face culling (RS:211) rejects every one of them, so the skip is exact.  A ray
 *                        that leaves a closed mesh no longer walks the boxes around its origin down to their leaves.  The counting
 *                        instantiation ("count_stats") and "qnodes" walk without it.  See urt_debug_read_scene_cones),
 *          "tile_entry" (-1 auto, the default | 0 off | 1 on: kernel_mode 3 on a scene of one MeshObject and no spheres.  While an image
 *                        accumulates the camera stands still, and all camera rays of an 8x8 tile descend the triangle BVH through the same
 *                        ancestors.  A pre-pass walks that common part once per tile — dropping the children whose box lies outside the
 *                        tile's frustum or whose normal cone faces away from all of its rays — and leaves up to 8 entry nodes per tile, 32 B;
 *                        camera rays start there instead of at the root.  Used by a launch whose frames all have the same camera matrices,
 *                        bit for bit, and pixel offsets in [0, 1]; the table is kept until the camera, the image size or the BVH changes.
 *                        auto builds a table only for a camera that has stood still — a launch of two frames or more, or the camera of the
 *                        previous launch — so that a camera that moves with every submitted frame pays no pre-pass; 1 builds it at once.
 *                        Not in the counting instantiation, not with "qnodes".  csrc/tile_entry.h; see urt_debug_read_tile_entry and
 *                        urt_launch_info::tile_entry),
 *          "refit" (0/1, default 1: moved and deformed MeshObjects are refitted on the GPU instead of rebuilt — see urt_debug_refit_stats;
 *                   0 turns the in-place update off altogether),
 *          "refit_vertices" (0/1, default 1: a SetData that changes elements of _Vertices / _Normals — same counts, _Indices untouched — is
 *                            taken in place: only the changed element range is copied to the device, and the MeshObjects whose vertex
 *                            span it meets are refitted / get their shading normals re-gathered; 0 = such a change prepares from scratch,
 *                            matrix moves are still refitted — see urt_debug_deform_stats),
 *          "prepare_device" (0/1, default 0: 1 = a full preparation reads _Vertices / _Indices / _Normals from their device mirrors (a buffer
 *                            without one is uploaded from its host copy, which is current then): no download of the three and no host
 *                            pass over them, their stale ranges and download counters stay as they are.  The triangle BVHs are then
 *                            always built on the GPU — by the builder "blas_builder" names when it is >= 1, else by 3 — and the
 *                            MeshObjects' vertex spans come from csrc/index_span.hip; same pixels.  See "the device side of a
 *                            ComputeBuffer", urt_debug_scene_vertex_spans and urt_debug_prepare_stats),
 *          "refit_rebuild_pct" (0, the default = never | > 100: when the surface-area cost of a deformed MeshObject's refitted tree exceeds
 *                               pct / 100 x the cost it had at the last full preparation, the in-place update is abandoned and the scene is
 *                               prepared from scratch — see urt_debug_scene_cost),
 *          "watchdog_cap" (test hook: scheduler trips a wave may make before it gives up; 0 = auto = 2^24 x frames of the launch x
 *                          max(1, numRays x numBounces / 8))
 *          — tuning knobs; they change speed only, never pixels. */
URT_API int urt_set_option(urt_context* ctx, const char* name, int value);
URT_API int urt_get_counters(urt_context* ctx, urt_counters* out);   /* synchronises */
URT_API int urt_reset_counters(urt_context* ctx);

/* ---- device groups: one host thread, N GPUs (SURVEY.md 8b "device list for 1/2/4/8 GPUs", 8e) ------------------------------
 * The reference issues everything from Unity's main thread to one GPU (RM:806-810).  A host that wants the frame
 * tile-partitioned over the GPUs of a node keeps its call sequence and swaps urt_* for urt_group_*:
 *  - scene buffers, uniforms, textures, options and Graphics.Blit calls are REPLICATED on every rank's context (one handle
 *    value names the same object on every rank);
 *  - urt_group_shader_dispatch gives rank r the 8-row strips r, r+N, ... with global pixel ids (= urt_shader_dispatch_rows):
 *    the union over the ranks is bit-identical to one full dispatch;
 *  - accumulation stays local to the ranks' strips; urt_group_gather is the ONE exchange per frame: strips of `src_texture`
 *    from every rank -> the full image `dst_texture` on rank 0 (pack kernels + hipMemcpyPeerAsync over xGMI, point-to-point
 *    to the root, ordered by events, no host synchronisation; queued behind the ranks' batched frames and submitted in
 *    bursts of up to 16);
 *  - readback, synchronize and counters act on the whole group (pixels come from rank 0).
 * The device list may repeat an ordinal (several ranks on one card).  urt_group_context exposes a rank's context for
 * per-rank inspection; objects must be created through the group. */
typedef struct urt_group urt_group;
URT_API int urt_group_create(const int* devices, int n_devices, urt_group** out_group);
URT_API int urt_group_destroy(urt_group* group);
URT_API int urt_group_size(urt_group* group);
URT_API urt_context* urt_group_context(urt_group* group, int rank);
URT_API const char* urt_group_last_error(urt_group* group);          /* group may be NULL for create failures */
URT_API int urt_group_buffer_create(urt_group* group, int count, int stride, urt_handle* out_buffer);            /* RM:247 */
URT_API int urt_group_buffer_set_data(urt_group* group, urt_handle buffer, const void* data, int count);          /* RM:250 */
URT_API int urt_group_buffer_set_data_range(urt_group* group, urt_handle buffer, int first, const void* data, int count);
URT_API int urt_group_buffer_release(urt_group* group, urt_handle buffer);
URT_API int urt_group_texture_create(urt_group* group, int width, int height, urt_handle* out_texture);          /* RM:834-840 */
URT_API int urt_group_texture_set_pixels(urt_group* group, urt_handle texture, const float* rgba);
URT_API int urt_group_texture_get_pixels(urt_group* group, urt_handle texture, float* rgba);                     /* rank 0's image */
URT_API int urt_group_texture_release(urt_group* group, urt_handle texture);
URT_API int urt_group_shader_set_buffer(urt_group* group, int kernel, const char* name, urt_handle buffer);      /* RM:787-794 */
URT_API int urt_group_shader_set_texture(urt_group* group, int kernel, const char* name, urt_handle texture);    /* RM:776, 803 */
URT_API int urt_group_shader_set_matrix(urt_group* group, const char* name, const float* m16);                   /* RM:773-774 */
URT_API int urt_group_shader_set_vector(urt_group* group, const char* name, const float* v4);                    /* RM:777 */
URT_API int urt_group_shader_set_float(urt_group* group, const char* name, float value);                         /* RM:778 */
URT_API int urt_group_shader_set_int(urt_group* group, const char* name, int value);                             /* RM:780-784 */
URT_API int urt_group_set_option(urt_group* group, const char* name, int value);
URT_API int urt_group_shader_dispatch(urt_group* group, int kernel, int groups_x, int groups_y, int groups_z);   /* RM:806-810, partitioned */
URT_API int urt_group_blit_add(urt_group* group, urt_handle src, urt_handle dst, float sample);                  /* RM:817-818 */
URT_API int urt_group_blit(urt_group* group, urt_handle src, urt_handle dst);                                    /* RM:819 */
URT_API int urt_group_gather(urt_group* group, urt_handle src_texture, urt_handle dst_texture);
URT_API int urt_group_flush(urt_group* group);
URT_API int urt_group_synchronize(urt_group* group);
URT_API int urt_group_get_counters(urt_group* group, urt_counters* out);   /* summed over the ranks; dispatches/launches/trace_ms = the largest rank's */
URT_API int urt_group_reset_counters(urt_group* group);

/* ---- host-side scene preparation (no GPU needed) ---------------------- */
/* Common to the urt_host_* helpers of this and the next two sections.  URT_ERR_INVALID_ARGUMENT: a negative count, a NULL array with a
 * positive count, an output capacity that is too small — checked first, nothing is written.  URT_ERR_SCENE: a record that points
 * outside the arrays (a MeshObject range outside the indices, an index outside the vertices); it is found while the records are
 * walked, so outputs that belong to earlier records (leaf boxes of earlier MeshObjects, lines already in a file) may have been written,
 * never more than the stated size of an output.  Non-finite and denormal coordinates are data, not errors.  Every failing call leaves a
 * non-empty message for the section's *_last_error(). */
/* RayTraceMaster.ComputeNormals (RM:340-368): per-vertex sum of the un-normalised face normals of every index slot whose
 * vertex POSITION equals this vertex's (weld across all meshes), in ascending slot order, then Vector3.Normalize —
 * O(V + I) by position hashing instead of the reference's O(V * I).  out_normals = 3 * n_vertices floats. */
URT_API int urt_host_compute_normals(const float* vertices, int n_vertices, const int32_t* indices, int n_indices,
                                     float* out_normals);
/* SetupBVHLeaves(List<MeshObject>) (RM:405-433): one world-space box per MeshObject (112-B records).  literal != 0 keeps
 * the reference's quirks (box seeded from _vertices[_indices[0]], the mesh's own first index slot skipped, A.7);
 * literal == 0 gives the tight box.  NULL vertices or indices with a positive count: URT_ERR_INVALID_ARGUMENT.  Boxes are a plain
 * loop of lo = min(lo, p), hi = max(hi, p) in that argument order (a NaN coordinate is skipped unless it comes first). */
URT_API int urt_host_mesh_leaf_bounds(const void* mesh_objects, int n_meshes, const float* vertices, int n_vertices,
                                      const int32_t* indices, int n_indices, int literal, urt_BVHNode* out_leaves);
/* SetupBVHLeaves(List<Sphere>) (RM:436-455): literal != 0 keeps the inverted boxes (vmin = pos + r, vmax = pos - r). */
URT_API int urt_host_sphere_leaf_bounds(const void* spheres, int n_spheres, int literal, urt_BVHNode* out_leaves);
/* CreateBVH's output contract (RM:681-722): implicit heap of 2^D - 1 nodes, D = ceil(log2 n) + 1, children 2i+1 / 2i+2,
 * interior and filler nodes index -1 (fillers all-zero, RM:490-494).  This one builds the tree by a deterministic median split
 * (O(n log n)); urt_host_build_object_bvh_pairing below is the reference's own O(n^3) pairing heuristic.  Pixels do not depend on
 * which of the two made the heap.  urt_host_object_bvh_length: 0 for n_objects <= 0, and -1 where 2^D - 1 does not fit in an int
 * (n_objects > 2^30); both builders answer a negative length, like a capacity below the length, with URT_ERR_INVALID_ARGUMENT.  The
 * median split takes any coordinates (a NaN centre sorts after every number; every leaf still appears exactly once). */
URT_API int urt_host_object_bvh_length(int n_objects);
URT_API int urt_host_build_object_bvh(const urt_BVHNode* leaves, int n_objects, urt_BVHNode* out_nodes, int capacity);
/* The reference's OWN builder restated literally — SetupBVHRankList / PairBVHBounds / JoinBVH / CreateBVH (RM:459-722): nearest-
 * neighbour ranking with "forbidden" pairs last, greedy pairing from start index n-1 (the volume comparison is dead code: the
 * candidate list is aliased, RM:670), lone trees joined under a copy of their own root, layers woven into the implicit heap.
 * Only the order of exact ties in the ranking sort (an unstable List.Sort in the reference) is this library's choice (stable).
 * A leaf with a NaN or infinite corner is URT_ERR_SCENE, nothing written: the reference's FindIndex (Vector3 ==) cannot find such a box
 * and its pairing throws.  A lone tree is joined with nothing under a copy of its root, so an interior node may have one filler child
 * and an object's leaf may appear a second time on an interior position. */
URT_API int urt_host_build_object_bvh_pairing(const urt_BVHNode* leaves, int n_objects, urt_BVHNode* out_nodes, int capacity);
/* The motion tables of urt_reproject_objects from the object lists before and after a move (n entries of _MeshObjects / _Spheres
 * each), entry i = current world -> previous world of object i.  Mesh: prevL * inverse(curL) of the two localToWorldMatrix fields
 * (their affine 3 x 4 parts), computed in float64 and rounded once to float32.  Sphere: linear part (r_prev / r_cur) * I, translation
 * c_prev - (r_prev / r_cur) * c_cur.  An object whose previous and current fields (the matrix; position and radius) are bit for bit
 * equal gets the exact identity bits, which is what urt_reproject_objects calls "not moved".  A singular curL or r_cur <= 0 gives an
 * all-NaN entry (that object then has no history) and is not an error.  URT_ERR_INVALID_ARGUMENT: n < 0, or a NULL pointer with n > 0. */
URT_API int urt_host_mesh_motion(const void* prev_mesh_objects, const void* cur_mesh_objects, int n, urt_ObjectMotion* out);
URT_API int urt_host_sphere_motion(const void* prev_spheres, const void* cur_spheres, int n, urt_ObjectMotion* out);
/* The message of the calling thread's last failing call of this section; the pointer stays valid until that thread's next failing
 * call of the section. */
URT_API const char* urt_host_last_error(void);

/* ---- host-side image I/O (no GPU needed) ---------------------------------- */
/* Radiance RGBE (.hdr, FORMAT=32-bit_rle_rgbe, flat or new-style RLE scanlines) -> RGBA32F, row 0 = bottom: the pixels a
 * caller hands to urt_texture_set_pixels for "_SkyboxTexture" (RM:776).  out_rgba == NULL queries the size.  Sizes 1..65536; new-style
 * RLE where the width is 8..32767, flat rows otherwise; header lines of up to 4096 bytes.  URT_ERR_INVALID_ARGUMENT: a NULL or
 * unopenable path, capacity_floats below width * height * 4 (nothing is written).  URT_ERR_LAYOUT: anything that is not such a file,
 * or one that ends early or whose runs overrun a row; *out_width / *out_height are set once the header is read, rows decoded before the
 * fault stay in out_rgba, and never more than width * height * 4 floats are written.  URT_OK: exactly those floats, alpha 1. */
URT_API int urt_host_load_hdr(const char* path, int* out_width, int* out_height, float* out_rgba, size_t capacity_floats);
/* RGBA32F image -> RGBA32F image of another size with a separable Mitchell-Netravali filter: the importer step the reference's sky
 * assets go through (`maxTextureSize: 2048`, `resizeAlgorithm: 0`, Assets/Skyboxes/CloudedSunGlow4k.hdr.meta:36,73).  An approximation
 * of Unity's closed-source resampler (its BC6H compression is not reproduced).  Output texel d takes the source texels floor(c - s) ..
 * ceil(c + s) around c = (d + 0.5) * scale - 0.5 with s = 2 * max(1, scale), indices clamped to the edge, weights
 * Mitchell((k - c) / max(1, scale)) normalised to sum 1 (evaluated in double, rounded once), rows first, then columns; sums in float32.
 * Sides 1 .. 2^28. */
URT_API int urt_host_resize_rgba(const float* src, int width, int height, float* dst, int new_width, int new_height);
/* RGBA32F image (row 0 = bottom) -> .pfm (float RGB, bottom row first). */
URT_API int urt_host_write_pfm(const char* path, const float* rgba, int width, int height);
/* RGBA32F linear image -> 8-bit sRGB .png (what ScreenCapture.CaptureScreenshot produces for RM:762). */
URT_API int urt_host_write_png(const char* path, const float* rgba, int width, int height);
/* The PNG writer's pixel encoding on its own: RGBA32F linear -> RGBA8 (colour: sRGB transfer function, clamped, NaN -> 0; alpha: UNORM8),
 * and the encoder as the step function it is: out256[k] = the smallest float whose code is >= k (out256[0] = -inf) — the table the GPU
 * encoder of urt_texture_read_begin_format searches. */
URT_API int urt_host_encode_srgb8(const float* rgba, size_t n_pixels, unsigned char* out_rgba8);
URT_API int urt_host_srgb8_first_floats(float* out256);
/* As urt_host_last_error, for this section: per thread, valid until the same thread's next failing call of the section. */
URT_API const char* urt_host_io_last_error(void);

/* ---- host-side debug log and BVH inspection (no GPU needed) ------------------ */
/* RayTraceDebug.Log (RD:25-36): appends `text` + newline to the file when level <= debug_level.  Returns URT_OK when
 * written, 1 when filtered by the level (the reference's Log returns 1 then as well). */
URT_API int urt_host_log(const char* path, int debug_level, int level, const char* text);
/* The five count lines of RebuildObjectLists (RM:331-335): "# of Spheres: n", "# of Mesh Objects: n", ... at level 2. */
URT_API int urt_host_log_scene_counts(const char* path, int debug_level, int n_spheres, int n_mesh_objects, int n_vertices,
                                      int n_indices, int n_normals);
/* The two reports of RebuildTrees (RM:731-735): amount, depth, complete length 2^depth - 1, real length — at level 2. */
URT_API int urt_host_log_tree_report(const char* path, int debug_level, int n_mesh_objects, int mesh_depth, int mesh_real_length,
                                     int n_spheres, int sphere_depth, int sphere_real_length);
/* Text stand-in for the editor gizmos of RayTraceDebug.DrawBVH (RD:92-117): walks `depth` levels of the implicit heap from the
 * root (children 2i+1 / 2i+2, pre-order) and writes one line per node: "(position in list, object index)" as the gizmo labels
 * it (RD:108), the box, its centre, and " [ray]" when the test segment start -> end passes RD's CPU slab test (RD:70-89; the
 * gizmo paints those boxes black).  ray_start3 / ray_end3 may both be NULL.  out_lines = nodes written. */
URT_API int urt_host_dump_bvh(const char* path, const urt_BVHNode* nodes, int n_nodes, int depth, const float* ray_start3,
                              const float* ray_end3, int* out_lines);
/* Text stand-in for RayTraceDebug.DrawNormals (RD:165-183): per index slot of every MeshObject the gizmo's base point
 * MultiplyPoint3x4(_vertices[_indices[i]]) and the tip of its line MultiplyPoint3x4(_vertices[_indices[i]] + _normals[_indices[i]] * 0.1f),
 * one line "mesh slot (base) -> (tip)".  out_lines = slots written. */
URT_API int urt_host_dump_normals(const char* path, const void* mesh_objects, int n_meshes, const float* vertices, int n_vertices,
                                  const int32_t* indices, int n_indices, const float* normals, int n_normals, int* out_lines);
/* As urt_host_last_error, for this section: per thread, valid until the same thread's next failing call of the section.  A call
 * that fails on its arguments creates no file and sets *out_lines to 0. */
URT_API const char* urt_host_debug_last_error(void);

/* ---- introspection for tests (host only, no GPU needed) ------------------------------------ */
/* Run the library's triangle-BVH builder — the one urt_shader_dispatch uses — over host copies of
 * _MeshObjects (112 B records), _Vertices, _Indices, and keep the result in a process-wide cache.
 * Reports the sizes.  tests/ use it to validate the BVH and to hand it to the oracle's culled mode. */
URT_API int urt_debug_build_blas(const void* mesh_objects, int n_meshes, const float* vertices, int n_vertices,
                                 const int32_t* indices, int n_indices, int* out_n_nodes, int* out_n_tris,
                                 int* out_max_depth);
/* Copy the cached BVH out: nodes = n_nodes * 16 floats (layout in DESIGN.md "BLAS"); tri_index = n_tris
 * index-slot numbers (i of RS:243) in leaf order; mesh_root / mesh_first_tri = one entry per MeshObject.
 * Any pointer may be NULL. */
URT_API int urt_debug_get_blas(float* nodes, int32_t* tri_index, int32_t* mesh_root, int32_t* mesh_first_tri);
/* The triangle BVH of the context's CURRENT device scene, whichever builder made it ("blas_builder" option): prepares the
 * scene if it is stale (as the next dispatch would).  scene_info reports sizes, the depth of the deepest leaf and the host
 * wall time the last preparation took; read_scene_blas copies the nodes (n_nodes x 16 floats), the index slot of every
 * leaf-order triangle and the MeshObject roots back from the GPU.  Any pointer may be NULL. */
URT_API int urt_debug_scene_info(urt_context* ctx, int* out_n_nodes, int* out_n_tris, int* out_max_depth, float* out_prepare_ms);
/* The last trace launch of this context (deferred frames are submitted first): which kernel instantiation ran — by the name rocprofv3
 * prints for it, so that bench.py and the profile reducers name the kernel that really ran instead of re-deriving the dispatch logic —,
 * its grid, its dynamic LDS and what the frame batching did (slab_frames_max < the requested batch, or slab_out_of_memory: the Result
 * slots did not fit and the batch was halved / switched off, frame_batch.cpp ensure_slab).  No counterpart in the reference (one Dispatch
 * per frame, RM:806-810); measurement only. */
typedef struct urt_launch_info {
  char kernel[96];            /* e.g. "k_sched<false, 256, 0, false, false>" (COUNT, BLOCK, FMODE, MULTI, QN: kernels.hip) */
  int kernel_mode;            /* option "kernel_mode" the launch ran under (a degenerate dispatch runs mode 0) */
  int front_mode;             /* kernel_mode 3 / 5: 0 one mesh, 1 BVH top walked in the object-level phase, 2 listed, 3 masked */
  int count_stats;            /* the counting instantiation */
  int n_blocks, block_threads, lds_bytes, waves_per_cu;
  int n_frames, frame_group, xcd_run, tile_order, top_nodes, tlas_stack, blas_stack;
  int lds_tables;             /* bit 0 mesh heap, 1 sphere heap + spheres, 2 single-leaf triangle records, 3 walk table */
  int slab_frames, slab_frames_max, slab_out_of_memory;
  int experiment;             /* 1: the library is an A/B / probe / diagnostic build (negative urt_abi_version) */
  int blas_builder;           /* the triangle-BVH builder the scene's last full preparation used (0..3; what "blas_builder" -1 = auto resolved to) */
  int trace_stream;           /* 0: launched on the context's stream; 1 / 2: on one of the library's two trace streams (option "overlap_launches") */
  int slab_base;              /* first Result slot of the launch */
  int overlapped;             /* 1: the launch did not wait for the previous launch (it waited for the main stream as of the previous submission) */
  int overlapped_launches;    /* such launches since the context was created */
  int cones;                  /* 1: the launch's traversal applied the normal cones of option "blas_cones" (kernel_mode 3, not counting, no qnodes) */
  int handout;                /* kernel_mode 3: tiles per LDS reservation of a workgroup (option "handout": 1..16, a divisor of xcd_run); 0: every wave draws from the work counters */
  int tile_entry;             /* 1: the launch's camera rays started at the entries of a tile entry table (option "tile_entry") */
  int tile_entry_k;           /* entries per tile of that table (0: no table) */
} urt_launch_info;
URT_API int urt_debug_launch_info(urt_context* ctx, urt_launch_info* out_info);
URT_API int urt_debug_read_scene_blas(urt_context* ctx, float* nodes, int32_t* tri_index, int32_t* mesh_root);
/* The 32-byte quantized triangle-BVH nodes of option "qnodes" (prepares a stale scene first): out receives 2 + 2 n float4 — grid
 * origin.xyz and quality (the smallest MeshObject in cells), cell.xyz and 0, then one 32-byte node per float node (csrc/qnodes.hip).
 * *out_n_nodes = n, or 0 while "qnodes" is 0 (then nothing is written; out may be NULL to ask for n first).  *out_in_use = 1 when
 * the traversal loop of the default trace kernel reads them (qnodes = 1, or -1 and a fine enough grid), else 0. */
URT_API int urt_debug_read_scene_qnodes(urt_context* ctx, float* out, int* out_n_nodes, int* out_in_use);
/* The normal cones of option "blas_cones" as the trace kernel reads them (prepares a stale scene first): words = 2 n_nodes dwords, the cone
 * of child 0 and of child 1 of every node — four signed bytes (ax, ay, az, T), ax in the lowest; the child is skipped iff
 * ax rx + ay ry + az rz - 127 T > 0 for the ray's bytes r = round(127 d); 0 = no cone —, and tri_edges = 6 n_tris floats, e1.xyz and
 * e2.xyz of every leaf-order triangle of the world-space records the cones were derived from (what Moller-Trumbore reads).  Either may
 * be NULL.  *out_in_use = 1 when the words are filled in (the option is on and the scene has triangle BVHs), else they are all 0. */
URT_API int urt_debug_read_scene_cones(urt_context* ctx, uint32_t* words, float* tri_edges, int* out_in_use);
/* The tile entry table of option "tile_entry" as the last launch that used one read it (deferred frames are submitted first; synchronises):
 * *out_tiles_x x *out_tiles_y records, row by row over the 8x8 tiles of the whole image, *out_k dwords each — the node codes a camera ray
 * of the tile starts from (>= 0 an interior node of the triangle BVH, < 0 a leaf code), padded with 0x80000000; a record of padding alone
 * means that no camera ray of the tile can hit the mesh.  All three are 0 while the context holds no table.  out (may be NULL) receives at
 * most capacity_words dwords.  *out_builds: tables built since the context was created — a launch with the camera, image size and BVH
 * of the cached table builds none.  Any pointer may be NULL. */
URT_API int urt_debug_read_tile_entry(urt_context* ctx, int32_t* out, uint64_t capacity_words, int* out_tiles_x, int* out_tiles_y, int* out_k,
                                      uint64_t* out_builds);
/* Scene preparation of a context keeps the triangle BVH of every MeshObject and reuses it at the next preparation when the
 * MeshObject's matrix and the positions behind its index slots are unchanged (the reference re-uploads every buffer when
 * any object moves, RM:262-336).  Reports how many MeshObject BVHs were reused / built since the context was created. */
URT_API int urt_debug_blas_cache_stats(urt_context* ctx, uint64_t* out_reused, uint64_t* out_built);
/* The walk table the default kernel's masked object-level phase uses for a mesh heap of <= 31 nodes (DESIGN.md §5 "masked FRONT"): header
 * words (n_eval, levels, interior mask, exist mask | leaf_any, leaf_valid | 4 depth masks | 4 left-child shifts), 32 x {root, small_first}
 * per heap position in pop order, then n_eval x {vmin.xyz, parent bit | vmax.xyz, position bit}.  out_words = 0 when the heap does not
 * qualify (empty or > 31 nodes).  Host only: tests/test_walk_table.py checks the mask arithmetic against the literal walk RS:294-326. */
URT_API int urt_debug_build_walk_table(const urt_BVHNode* heap, int n_nodes, int n_meshes, const int32_t* mesh_root, const int32_t* small_first,
                                       float* out, int capacity_words, int* out_words);
/* Dynamic scenes.  When the only buffer CONTENTS that changed since the scene was prepared are those of _MeshObjects, _MeshBVH, _Spheres
 * and _SphereBVH (same counts, same index range per MeshObject; data equal to what a buffer already holds counts as unchanged — the
 * reference re-uploads every list when one object moves, RM:215-230 -> 262-336), the device scene is updated in place: materials and
 * object-level tables are re-packed, and MeshObjects whose localToWorldMatrix changed keep the topology of their triangle BVH — their
 * triangle records and boxes are recomputed on the GPU (csrc/refit.hip; option "refit" = 0 turns this off).  Reports MeshObjects
 * refitted and in-place preparations since the context was created.  A deformed MeshObject (changed _Vertices, urt_debug_deform_stats)
 * counts as refitted and its update as in place; a full preparation forced by "refit_rebuild_pct" counts as neither. */
URT_API int urt_debug_refit_stats(urt_context* ctx, uint64_t* out_refitted_meshes, uint64_t* out_incremental_preparations);
/* Deformation (option "refit_vertices"): a MeshObject is DEFORMED when the dirty element range of _Vertices meets the span of vertices its
 * index range refers to, and has its normals changed when the dirty range of _Normals does.
 * out6: deformed MeshObjects refitted, MeshObjects whose normals were re-gathered, vertex + normal bytes copied to the device by in-place
 * updates, full preparations forced by "refit_rebuild_pct" — all since the context was created; then the largest cost ratio of the last
 * in-place update as float bits, and 0 (reserved) */
URT_API int urt_debug_deform_stats(urt_context* ctx, uint64_t out6[6]);
/* The surface-area cost of every MeshObject's triangle BVH: the sum over its nodes and both children of area(child box) x (its triangle
 * count for a leaf, 1 for a node) / area(root box); 0 for a MeshObject without nodes or with a root box of zero or non-finite area.
 * per MeshObject: cost now and baseline cost (2 floats each); prepares a stale scene first */
URT_API int urt_debug_scene_cost(urt_context* ctx, float* out, int n_meshes);
/* The vertex spans the prepared scene holds: per MeshObject the signed minimum (out_lo) and maximum (out_hi) of
 * _Indices[indices_offset .. indices_offset + (indices_count / 3) * 3 - 1], INT32_MAX / -1 for a MeshObject with fewer than three indices.
 * A changed range of _Vertices / _Normals deforms the MeshObjects whose span it meets (option "refit_vertices").  The full preparation
 * computes them: on the host from the host copy of _Indices, with option "prepare_device" on the GPU from the scene's device copy.
 * Every entry is INT32_MAX / -1 when the scene kept none ("refit" = 0, or no triangles).  Prepares a stale scene first, as
 * urt_debug_scene_info does, and nothing more.  URT_ERR_INVALID_ARGUMENT: a NULL pointer, or n_meshes is not the scene's number of MeshObjects. */
URT_API int urt_debug_scene_vertex_spans(urt_context* ctx, int32_t* out_lo, int32_t* out_hi, int n_meshes);
/* Full preparations of this context: out4 = those completed since the context was created, those of them that option "prepare_device"
 * fed from device memory, the number of indices one work item of the vertex-span kernel scans (csrc/index_span.h kSpanChunk), and — as
 * float bits, in milliseconds, measured with events while option "time_dispatch" is on, else 0 — the device time of the last span pass.
 * Prepares nothing. */
URT_API int urt_debug_prepare_stats(urt_context* ctx, uint64_t out4[4]);
/* What the library holds right now, PROCESS-WIDE (every context and group of the process; needs none): out4 = device bytes, pinned host
 * bytes, events, streams.  Counts only the library's own holders (csrc/owned.h) — not external textures, the caller's streams or what
 * the HIP runtime keeps for itself.  A context or group that is destroyed gives back everything it took. */
URT_API int urt_debug_live_resources(uint64_t out4[4]);
/* kernel_mode 5 with "count_stats" = 1: what the shared traversal service did since the last urt_reset_counters —
 * out6 = visits of the service, its trips, active lanes summed over the trips, claim rounds, rays claimed, rays suspended. */
URT_API int urt_debug_serve_stats(urt_context* ctx, unsigned long long* out6);

#ifdef __cplusplus
}
#endif
