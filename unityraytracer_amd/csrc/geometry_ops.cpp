// geometry_ops.cpp — the entry points of include/urt.h that read and write ComputeBuffers on the device with kernels of their own: skinning,
// buffer bounds, the object-level BVH, normals plans and morph plans.  They work on the buffers' device mirrors (context.cpp buffer_mirror) and
// mark what they wrote (mark_device_written).  Every argument is checked first: on an error nothing is mirrored, enqueued or marked.
#include "experiments.h"
#include "context_impl.h"

#include <limits>

#include "morph.h"
#include "morph_plan.h"
#include "normals.h"
#include "normals_plan.h"
#include "object_bvh.h"
#include "skin.h"

using namespace urtd;

namespace urtd {

int resolve_buffers(urt_context* ctx, const char* who, const BufArg* a, int n, Buffer** b) {
  for (int k = 0; k < n; k++) {
    b[k] = a[k].absent ? nullptr : find_buffer(ctx, a[k].h);
    if (!b[k] && !a[k].absent) return fail(ctx, URT_ERR_INVALID_HANDLE, std::string(who) + ": " + a[k].name + " is 0 or an unknown buffer handle");
  }
  for (int k = 0; k < n; k++)
    if (b[k] && b[k]->stride != a[k].stride) return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string(who) + ": the stride of " + a[k].name + " is not " + std::to_string(a[k].stride));
  return URT_OK;
}

int mirror_buffers(urt_context* ctx, Buffer* const* b, int n) {
  for (int k = 0; k < n; k++) if (b[k]) if (int rc = buffer_mirror(ctx, *b[k])) return rc;
  return URT_OK;
}

// The checks of a call whose inputs a[0 .. first_dst) and destinations a[first_dst .. n) go together: resolve_buffers, then every buffer
// has the count of a[0] but for the bits of `loose`, then no input is a destination (`article`: the message's "a" or "the" destination).
static int check_buffers(urt_context* ctx, const char* who, const BufArg* a, int n, Buffer** b, unsigned int loose, int first_dst, const char* article) {
  if (int rc = resolve_buffers(ctx, who, a, n, b)) return rc;
  for (int k = 1; k < n; k++)
    if (b[k] && !((loose >> k) & 1u) && b[k]->count != b[0]->count) return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string(who) + ": the count of " + a[k].name + " is not that of " + a[0].name);
  for (int k = 0; k < first_dst; k++)
    for (int j = first_dst; j < n; j++)
      if (b[k] && b[j] && a[k].h == a[j].h) return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + a[k].name + " is also " + article + " destination");
  return URT_OK;
}

// ... of urt_skin_vertices and urt_morph_vertices: a[0] rest_vertices, a[1] rest_normals, a[n - 2] dst_vertices, a[n - 1] dst_normals, the two
// normals buffers absent together (a rest_normals given all the same must at least exist); a[loose] has a count of its own.
static int check_deform_buffers(urt_context* ctx, const char* who, const BufArg* a, int n, Buffer** b, int loose) {
  if (a[1].absent && a[1].h && !find_buffer(ctx, a[1].h)) return fail(ctx, URT_ERR_INVALID_HANDLE, std::string(who) + ": rest_normals is an unknown buffer handle");
  if (int rc = check_buffers(ctx, who, a, n, b, 1u << loose, n - 2, "a")) return rc;
  if (b[n - 1] && a[n - 1].h == a[n - 2].h) return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string(who) + ": dst_vertices and dst_normals are one buffer");
  return URT_OK;
}

// Plans (ctx->normals_plans, ctx->morph_plans): the plan of a handle, or null with the error set
template <typename Plans>
static typename Plans::mapped_type* find_plan(urt_context* ctx, Plans& plans, urt_handle plan, const char* who) {
  auto it = plans.find(plan);
  if (it != plans.end()) return &it->second;
  fail(ctx, URT_ERR_INVALID_HANDLE, std::string(who) + ": unknown plan handle");
  return nullptr;
}

template <typename Plans>
static int release_plan(urt_context* ctx, Plans& plans, urt_handle plan, const char* who) {
  auto* d = find_plan(ctx, plans, plan, who);
  if (!d) return URT_ERR_INVALID_HANDLE;
  if (d->info.device_bytes) {                                // kernels queued on the stream may still read the plan
    URT_HIP(ctx, hipSetDevice(ctx->device));
    URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  }
  plans.erase(plan);
  return URT_OK;
}

// One array of a plan goes to the device (an empty one stays unallocated).  A failure leaves through the holders: nothing stays allocated.
template <typename T>
static hipError_t upload(DeviceBuf<T>& buf, const std::vector<T>& host, uint64_t& device_bytes) {
  if (host.empty()) return hipSuccess;
  const size_t bytes = host.size() * sizeof(T);
  if (hipError_t e = buf.alloc(host.size())) return e;
  device_bytes += bytes;
  return hipMemcpy(buf.get(), host.data(), bytes, hipMemcpyHostToDevice);
}

}  // namespace urtd

extern "C" {

int urt_skin_vertices(urt_context* ctx, const urt_SkinBuffers* in, int first, int count, urt_handle dst_vertices, urt_handle dst_normals) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!in) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "skin_vertices: in is NULL");
  URT_GUARD_BEGIN
  const bool normals = dst_normals != 0;
  if (normals && !in->rest_normals) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "skin_vertices: dst_normals without rest_normals");
  enum { kRestV, kRestN, kIdx, kWgt, kBones, kDstV, kDstN, kArgs };
  const BufArg a[kArgs] = {{in->rest_vertices, "rest_vertices", 12}, {in->rest_normals, "rest_normals", 12, !normals}, {in->bone_indices, "bone_indices", 16},
                           {in->bone_weights, "bone_weights", 16}, {in->bones, "bones", (int)sizeof(urt_ObjectMotion)},
                           {dst_vertices, "dst_vertices", 12}, {dst_normals, "dst_normals", 12, !normals}};
  Buffer* b[kArgs];
  if (int rc = check_deform_buffers(ctx, "skin_vertices", a, kArgs, b, kBones)) return rc;
  if (int rc = check_element_range(ctx, "skin_vertices", *b[kRestV], first, count)) return rc;
  if (count == 0) return URT_OK;
  if (int rc = mirror_buffers(ctx, b, kArgs)) return rc;
  URT_HIP(ctx, skin_vertices((const float*)b[kRestV]->mirror.get(), normals ? (const float*)b[kRestN]->mirror.get() : nullptr,
                             (const int32_t*)b[kIdx]->mirror.get(), (const float*)b[kWgt]->mirror.get(), (const float*)b[kBones]->mirror.get(),
                             b[kBones]->count, first, count, (float*)b[kDstV]->mirror.get(), normals ? (float*)b[kDstN]->mirror.get() : nullptr, touch(ctx)));
  mark_device_written(ctx, dst_vertices, *b[kDstV], first, count);
  if (normals) mark_device_written(ctx, dst_normals, *b[kDstN], first, count);
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_buffer_bounds(urt_context* ctx, urt_handle buffer, int first, int count, float out6[6], int* out_n) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  Buffer* b = find_buffer(ctx, buffer);
  if (!b) return fail(ctx, URT_ERR_INVALID_HANDLE, "buffer_bounds: unknown buffer handle");
  if (b->stride != 12) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "buffer_bounds: the stride of the buffer is not 12");
  if (int rc = check_element_range(ctx, "buffer_bounds", *b, first, count)) return rc;
  if (!out6) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "buffer_bounds: out6 is NULL");
  URT_GUARD_BEGIN
  const float inf = std::numeric_limits<float>::infinity();
  for (int c = 0; c < 3; c++) { out6[c] = inf; out6[3 + c] = -inf; }
  if (out_n) *out_n = 0;
  if (count == 0) return URT_OK;
  if (int rc = buffer_mirror(ctx, *b)) return rc;
  URT_HIP(ctx, hipSetDevice(ctx->device));
  const size_t words = (size_t)(kBoundsMaxBlocks + 1) * kBoundsWords;
  if (int rc = reserve(ctx, ctx->bd_partial, words, "buffer_bounds: scratch allocation", ctx->stream)) return rc;
  if (!ctx->bd_result) URT_HIP(ctx, ctx->bd_result.alloc(kBoundsWords));
  float* d_out = ctx->bd_partial.get() + (size_t)kBoundsMaxBlocks * kBoundsWords;
  URT_HIP(ctx, buffer_bounds((const float*)b->mirror.get(), first, count, ctx->bd_partial.get(), d_out, touch(ctx)));
  URT_HIP(ctx, hipMemcpyAsync(ctx->bd_result.get(), d_out, kBoundsWords * sizeof(float), hipMemcpyDeviceToHost, touch(ctx)));
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  std::memcpy(out6, ctx->bd_result.get(), 6 * sizeof(float));
  uint32_t n = 0;
  std::memcpy(&n, ctx->bd_result.get() + 6, 4);
  if (out_n) *out_n = (int)n;
  return check_watchdog(ctx);
  URT_GUARD_END(ctx)
}

/* ---- the object-level BVH on the device (include/urt.h; csrc/object_bvh.hip) ---- */
static_assert(URT_OBJECT_BVH_DEVICE_MAX == urtd::kObjectBvhDeviceMax && URT_MESH_LEAF_BLOCKS == urtd::kMeshLeafBlocks, "include/urt.h: the constants of csrc/object_bvh.h");

int urt_mesh_leaf_bounds_device(urt_context* ctx, urt_handle mesh_objects, urt_handle vertices, urt_handle indices, urt_handle dst_leaves) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  enum { kMeshes, kVerts, kIdx, kDst, kArgs };
  const BufArg a[kArgs] = {{mesh_objects, "mesh_objects", URT_STRIDE_MESHOBJECT}, {vertices, "vertices", URT_STRIDE_VEC3}, {indices, "indices", URT_STRIDE_INDEX},
                           {dst_leaves, "dst_leaves", URT_STRIDE_BVHNODE}};
  Buffer* b[kArgs];
  if (int rc = check_buffers(ctx, "mesh_leaf_bounds_device", a, kArgs, b, (1u << kVerts) | (1u << kIdx), kDst, "the")) return rc;
  const int n = b[kMeshes]->count;
  if (n == 0) return URT_OK;
  if (int rc = buffer_sync_host(ctx, *b[kMeshes])) return rc;   // the ranges are validated where the host can read them
  for (int m = 0; m < n; m++) {
    urt_MeshObject mo;
    std::memcpy(&mo, b[kMeshes]->host.data() + (size_t)m * sizeof mo, sizeof mo);
    if (mo.indices_offset < 0 || mo.indices_count < 0 || (long long)mo.indices_offset + (long long)mo.indices_count > (long long)b[kIdx]->count)
      return fail(ctx, URT_ERR_SCENE, "mesh_leaf_bounds_device: MeshObject " + std::to_string(m) + " names a range outside indices");
  }
  URT_HIP(ctx, hipSetDevice(ctx->device));
  const size_t rows = (size_t)std::min(n, 65535);
  if (int rc = reserve(ctx, ctx->ob_partial, rows * kMeshLeafBlocks * kMeshLeafWords, "mesh_leaf_bounds_device: scratch allocation", ctx->stream)) return rc;
  if (int rc = mirror_buffers(ctx, b, kArgs)) return rc;
  URT_HIP(ctx, mesh_leaf_bounds(b[kMeshes]->mirror.get(), n, (const float*)b[kVerts]->mirror.get(), b[kVerts]->count,
                                (const int32_t*)b[kIdx]->mirror.get(), b[kIdx]->count, ctx->ob_partial.get(), b[kDst]->mirror.get(), touch(ctx)));
  mark_device_written(ctx, dst_leaves, *b[kDst], 0, n);
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_sphere_leaf_bounds_device(urt_context* ctx, urt_handle spheres, urt_handle dst_leaves) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  const BufArg a[2] = {{spheres, "spheres", URT_STRIDE_SPHERE}, {dst_leaves, "dst_leaves", URT_STRIDE_BVHNODE}};
  Buffer* b[2];
  if (int rc = check_buffers(ctx, "sphere_leaf_bounds_device", a, 2, b, 0, 1, "the")) return rc;
  const int n = b[0]->count;
  if (n == 0) return URT_OK;
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = mirror_buffers(ctx, b, 2)) return rc;
  URT_HIP(ctx, sphere_leaf_bounds(b[0]->mirror.get(), n, b[1]->mirror.get(), touch(ctx)));
  mark_device_written(ctx, dst_leaves, *b[1], 0, n);
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_build_object_bvh_device(urt_context* ctx, urt_handle leaves, urt_handle dst_nodes) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  const BufArg a[2] = {{leaves, "leaves", URT_STRIDE_BVHNODE}, {dst_nodes, "dst_nodes", URT_STRIDE_BVHNODE}};
  Buffer* b[2];
  if (int rc = check_buffers(ctx, "build_object_bvh_device", a, 2, b, ~0u, 1, "the")) return rc;   // (the count of dst_nodes: below)
  const int n = b[0]->count;
  if (n > URT_OBJECT_BVH_DEVICE_MAX)
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "build_object_bvh_device: more than " + std::to_string(URT_OBJECT_BVH_DEVICE_MAX) +
                                                   " leaves: build this heap with urt_host_build_object_bvh");
  const int len = urt_host_object_bvh_length(n);
  if (b[1]->count != len) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "build_object_bvh_device: the count of dst_nodes is not urt_host_object_bvh_length(" + std::to_string(n) + ") = " + std::to_string(len));
  if (n == 0) return URT_OK;
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = mirror_buffers(ctx, b, 2)) return rc;
  URT_HIP(ctx, build_object_bvh(b[0]->mirror.get(), n, b[1]->mirror.get(), len, touch(ctx)));
  mark_device_written(ctx, dst_nodes, *b[1], 0, len);
  return URT_OK;
  URT_GUARD_END(ctx)
}

/* ---- normals on the device (include/urt.h; csrc/normals_plan.h, csrc/normals.hip) ---- */
int urt_normals_plan_create(urt_context* ctx, urt_handle vertices, urt_handle indices, int first, int count, urt_handle* out_plan) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!out_plan) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "normals_plan_create: out_plan is NULL");
  *out_plan = 0;
  URT_GUARD_BEGIN
  const BufArg a[2] = {{vertices, "vertices", 12}, {indices, "indices", 4}};
  Buffer* b[2];
  if (int rc = resolve_buffers(ctx, "normals_plan_create", a, 2, b)) return rc;
  Buffer *v = b[0], *ix = b[1];
  if (ix->count % 3 != 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "normals_plan_create: the count of indices is not a multiple of 3");
  if (int rc = check_element_range(ctx, "normals_plan_create", *v, first, count)) return rc;
  if (int rc = buffer_sync_host(ctx, *v)) return rc;         // the weld is found from the buffers' contents NOW
  if (int rc = buffer_sync_host(ctx, *ix)) return rc;
  NormalsPlan plan;
  if (normals_plan_build((const float*)v->host.data(), v->count, (const int32_t*)ix->host.data(), ix->count, first, count, plan) != kNormalsPlanOk)
    return fail(ctx, URT_ERR_SCENE, "normals_plan_create: index outside _Vertices");
  DevNormalsPlan d;
  d.vertices = vertices; d.n_vertices = v->count;
  d.info = {first, count, plan.n_lists, (int)(plan.tris.size() / 3), (int)plan.entries.size(), plan.max_valence, 0};
  URT_HIP(ctx, hipSetDevice(ctx->device));
  URT_HIP(ctx, upload(d.tris, plan.tris, d.info.device_bytes));
  URT_HIP(ctx, upload(d.entries, plan.entries, d.info.device_bytes));
  URT_HIP(ctx, upload(d.ranges, plan.ranges, d.info.device_bytes));
  const urt_handle h = ctx->next_id++;
  ctx->normals_plans.emplace(h, std::move(d));
  *out_plan = h;
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_normals_plan_info(urt_context* ctx, urt_handle plan, urt_NormalsPlanInfo* out) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  const DevNormalsPlan* d = find_plan(ctx, ctx->normals_plans, plan, "normals_plan_info");
  if (!d) return URT_ERR_INVALID_HANDLE;
  if (!out) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "normals_plan_info: out is NULL");
  *out = d->info;
  return URT_OK;
}

int urt_normals_plan_release(urt_context* ctx, urt_handle plan) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  return release_plan(ctx, ctx->normals_plans, plan, "normals_plan_release");
}

int urt_compute_normals(urt_context* ctx, urt_handle plan, urt_handle dst_normals) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  const DevNormalsPlan* d = find_plan(ctx, ctx->normals_plans, plan, "compute_normals");
  if (!d) return URT_ERR_INVALID_HANDLE;
  const urt_NormalsPlanInfo& p = d->info;
  Buffer* v = find_buffer(ctx, d->vertices);
  if (!v || v->count != d->n_vertices || v->stride != 12) return fail(ctx, URT_ERR_INVALID_HANDLE, "compute_normals: the plan's vertices buffer was released");
  const BufArg a = {dst_normals, "dst_normals", 12};
  Buffer* dst;
  if (int rc = resolve_buffers(ctx, "compute_normals", &a, 1, &dst)) return rc;
  if (dst->count != v->count) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "compute_normals: the count of dst_normals is not that of the vertices buffer");
  if (dst_normals == d->vertices) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "compute_normals: dst_normals is the vertices buffer");
  if (p.count == 0) return URT_OK;
  Buffer* const both[2] = {v, dst};
  if (int rc = mirror_buffers(ctx, both, 2)) return rc;
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = reserve(ctx, ctx->nm_face, (size_t)p.n_triangles, "compute_normals: scratch allocation", ctx->stream)) return rc;
  URT_HIP(ctx, compute_normals((const float*)v->mirror.get(), d->tris.get(), p.n_triangles, d->ranges.get(), d->entries.get(), p.first, p.count,
                               ctx->nm_face.get(), (float*)dst->mirror.get(), touch(ctx)));
  mark_device_written(ctx, dst_normals, *dst, p.first, p.count);
  return URT_OK;
  URT_GUARD_END(ctx)
}

/* ---- blend shapes on the device (include/urt.h; csrc/morph_plan.h, csrc/morph.hip) ---- */
static_assert(sizeof(urt_MorphDelta) == 32 && sizeof(urtd::MorphDeltaIn) == 32 && sizeof(urt_MorphPlanInfo) == 32, "include/urt.h: morph layouts");

int urt_morph_plan_create(urt_context* ctx, const urt_MorphDelta* deltas, int n_deltas, int n_targets, int first, int count, urt_handle* out_plan) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!out_plan) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "morph_plan_create: out_plan is NULL");
  *out_plan = 0;
  URT_GUARD_BEGIN
  if (n_deltas < 0 || count < 0 || first < 0 || (long long)first + (long long)count > 0x7fffffffLL)
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "morph_plan_create: a negative n_deltas, first or count, or a served range beyond 2^31 - 1");
  if (n_deltas > 0 && !deltas) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "morph_plan_create: deltas is NULL");
  if (n_targets < 1 || n_targets > kMorphMaxTargets) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "morph_plan_create: n_targets is outside 1..4096");
  const MorphDeltaIn* in = (const MorphDeltaIn*)deltas;
  MorphPlan plan;
  if (const int rc = morph_plan_build(in, n_deltas, n_targets, first, count, plan))
    return fail(ctx, URT_ERR_SCENE, rc == kMorphPlanBadVertex ? "morph_plan_create: a delta names a vertex outside the served range"
                                                               : "morph_plan_create: a delta names a target outside 0..n_targets-1");
  // the entries in plan order, as csrc/morph.hip reads them: this is the copy of `deltas`
  std::vector<int32_t> targets((size_t)n_deltas);
  std::vector<float> values(6 * (size_t)n_deltas);
  for (size_t e = 0; e < (size_t)n_deltas; e++) {
    const MorphDeltaIn& d = in[plan.order[e]];
    targets[e] = d.target;
    std::memcpy(&values[6 * e], d.dp, 12);
    std::memcpy(&values[6 * e + 3], d.dn, 12);
  }
  DevMorphPlan d;
  d.info = {first, count, n_targets, n_deltas, plan.max_valence, plan.n_touched, 0};
  URT_HIP(ctx, hipSetDevice(ctx->device));
  URT_HIP(ctx, upload(d.ranges, plan.ranges, d.info.device_bytes));
  URT_HIP(ctx, upload(d.targets, targets, d.info.device_bytes));
  URT_HIP(ctx, upload(d.deltas, values, d.info.device_bytes));
  const urt_handle h = ctx->next_id++;
  ctx->morph_plans.emplace(h, std::move(d));
  *out_plan = h;
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_morph_plan_info(urt_context* ctx, urt_handle plan, urt_MorphPlanInfo* out) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  const DevMorphPlan* d = find_plan(ctx, ctx->morph_plans, plan, "morph_plan_info");
  if (!d) return URT_ERR_INVALID_HANDLE;
  if (!out) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "morph_plan_info: out is NULL");
  *out = d->info;
  return URT_OK;
}

int urt_morph_plan_release(urt_context* ctx, urt_handle plan) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  return release_plan(ctx, ctx->morph_plans, plan, "morph_plan_release");
}

int urt_morph_vertices(urt_context* ctx, urt_handle plan, urt_handle rest_vertices, urt_handle rest_normals, urt_handle weights,
                       urt_handle dst_vertices, urt_handle dst_normals, int flags) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  const DevMorphPlan* d = find_plan(ctx, ctx->morph_plans, plan, "morph_vertices");
  if (!d) return URT_ERR_INVALID_HANDLE;
  const urt_MorphPlanInfo& p = d->info;
  if (flags & ~URT_MORPH_NORMALIZE) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "morph_vertices: unknown flags");
  const bool normals = dst_normals != 0;
  if ((flags & URT_MORPH_NORMALIZE) && !normals) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "morph_vertices: URT_MORPH_NORMALIZE without dst_normals");
  if (normals && !rest_normals) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "morph_vertices: dst_normals without rest_normals");
  enum { kRestV, kRestN, kWeights, kDstV, kDstN, kArgs };
  const BufArg a[kArgs] = {{rest_vertices, "rest_vertices", 12}, {rest_normals, "rest_normals", 12, !normals}, {weights, "weights", 4},
                           {dst_vertices, "dst_vertices", 12}, {dst_normals, "dst_normals", 12, !normals}};
  Buffer* b[kArgs];
  if (int rc = check_deform_buffers(ctx, "morph_vertices", a, kArgs, b, kWeights)) return rc;
  if (b[kWeights]->count != p.n_targets) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "morph_vertices: the count of weights is not the plan's n_targets");
  if (int rc = check_element_range(ctx, "morph_vertices", *b[kRestV], p.first, p.count)) return rc;
  if (p.count == 0) return URT_OK;
  if (int rc = mirror_buffers(ctx, b, kArgs)) return rc;
  URT_HIP(ctx, morph_vertices((const float*)b[kRestV]->mirror.get(), normals ? (const float*)b[kRestN]->mirror.get() : nullptr, d->ranges.get(),
                              d->targets.get(), d->deltas.get(), (const float*)b[kWeights]->mirror.get(), p.first, p.count,
                              (float*)b[kDstV]->mirror.get(), normals ? (float*)b[kDstN]->mirror.get() : nullptr,
                              (flags & URT_MORPH_NORMALIZE) != 0, touch(ctx)));
  mark_device_written(ctx, dst_vertices, *b[kDstV], p.first, p.count);
  if (normals) mark_device_written(ctx, dst_normals, *b[kDstN], p.first, p.count);
  return URT_OK;
  URT_GUARD_END(ctx)
}

}  // extern "C"
