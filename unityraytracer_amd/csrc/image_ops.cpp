// image_ops.cpp — the entry points of include/urt.h that work on whole images or ray batches next to the frame loop: ray queries,
// radiance queries, feature buffers, the denoiser, temporal reprojection, guide-driven upsampling, auto-exposure and tone mapping, depth of field,
// motion blur, bloom, resampling.
#include "experiments.h"
#include "context_impl.h"

#include "query.h"
#include "radiance.h"
#include "aov.h"
#include "denoise.h"
#include "reproject.h"
#include "resample.h"
#include "upsample.h"
#include "tonemap.h"
#include "dof.h"
#include "motion_blur.h"
#include "bloom.h"

using namespace urtd;

namespace {

// Checks the image-space entry points share; each caller runs them in its own order (it decides which error a doubly-wrong call reports).
struct TexArg { urt_handle h; const char* name; bool optional; };   // name NULL: the message names no argument

// t[k] = the texture of a[k] (NULL for an optional one that is not given).  dup_msg: a handle given twice fails with it.
int resolve_textures(urt_context* ctx, const char* prefix, const TexArg* a, int n, Texture** t, const char* dup_msg = nullptr) {
  for (int k = 0; k < n; k++) {
    t[k] = nullptr;
    if (a[k].optional && !a[k].h) continue;
    for (int j = 0; dup_msg && j < k; j++)
      if (a[j].h == a[k].h) return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string(prefix) + ": " + dup_msg);
    t[k] = find_texture(ctx, a[k].h);
    if (!t[k]) return fail(ctx, URT_ERR_INVALID_HANDLE, std::string(prefix) + ": unknown " + (a[k].name ? std::string(a[k].name) + " " : "") + "texture handle");
  }
  return URT_OK;
}

// every texture given has the size of t[0]
int check_same_size(urt_context* ctx, const char* prefix, Texture* const* t, int n) {
  for (int k = 1; k < n; k++)
    if (t[k] && (t[k]->w != t[0]->w || t[k]->h != t[0]->h)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string(prefix) + ": the textures differ in size");
  return URT_OK;
}

// the image kernels run 16 rows per workgroup and a grid holds 65535 of them
int check_height(urt_context* ctx, const char* prefix, const char* what, int height) {
  if ((height + 15) / 16 > 65535) return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string(prefix) + ": " + what + " taller than 1048560 pixels");
  return URT_OK;
}

// the outputs a[first..n) that are given are no other image of the call and not the sky
int check_outputs(urt_context* ctx, const char* prefix, const TexArg* a, int first, int n) {
  for (int k = first; k < n; k++) {
    if (!a[k].h) continue;
    for (int j = 0; j < n; j++)
      if (j != k && a[j].h == a[k].h)
        return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string(prefix) + ": the output " + a[k].name + " is also " + a[j].name);
    if (a[k].h == ctx->t_sky)
      return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string(prefix) + ": the output " + a[k].name + " is the texture bound as _SkyboxTexture");
  }
  return URT_OK;
}

// urt_radiance_query with option "radiance_persist" at -1: k_radiance_persist, measured faster on full-frame pixel batches in any order and
// within 1.5 % on the probe bake (profiles/r10_logs/r10_radiance_query_bench.log)
constexpr bool kRadiancePersistAuto = true;

// urt_select_pixels / urt_resample_below: the count texture fits the selection kernels (width * height <= 2^31 - 1: the total is an int)
int check_select_size(urt_context* ctx, const char* prefix, const Texture* c) {
  if ((size_t)c->w * (size_t)c->h > 0x7fffffffull)
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string(prefix) + ": the count texture has more than 2^31 - 1 texels");
  return URT_OK;
}

// the per-block counts of a selection over n_texels texels and the pinned word its total comes back in
int select_scratch(urt_context* ctx, const char* what, size_t n_texels) {
  if (int rc = reserve(ctx, ctx->rs_counts, select_scratch_words(n_texels), what, ctx->stream)) return rc;
  if (!ctx->rs_total) URT_HIP(ctx, ctx->rs_total.alloc(1, 64));
  return URT_OK;
}

// after launch_select_count (and whatever else was enqueued behind it): the call's one synchronisation; *total = the number selected
int select_total(urt_context* ctx, size_t n_texels, int* total) {
  URT_HIP(ctx, hipMemcpyAsync(ctx->rs_total.get(), ctx->rs_counts.get() + select_blocks(n_texels), sizeof(unsigned int), hipMemcpyDeviceToHost, touch(ctx)));
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  if (int rc = check_watchdog(ctx)) return rc;
  *total = (int)*ctx->rs_total.get();
  return URT_OK;
}

// weight and max_history of urt_blend_samples / urt_resample_below
int check_blend_numbers(urt_context* ctx, const char* prefix, float weight, float max_history) {
  if (!std::isfinite(weight) || !(weight > 0.0f)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string(prefix) + ": weight must be finite and > 0");
  if (!valid_max_history(max_history)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string(prefix) + ": max_history must be 0 or >= 1");
  return URT_OK;
}

// dst and count of urt_blend_samples / urt_resample_below: two known textures of one size, neither bound as the sky
int resolve_blend_targets(urt_context* ctx, const char* prefix, urt_handle dst, urt_handle count, Texture** t) {
  const TexArg a[2] = {{dst, "dst", false}, {count, "count", false}};
  if (int rc = resolve_textures(ctx, prefix, a, 2, t)) return rc;
  if (dst == count) return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string(prefix) + ": dst and count are the same texture");
  if (int rc = check_same_size(ctx, prefix, t, 2)) return rc;
  return check_outputs(ctx, prefix, a, 0, 2);
}

}  // namespace

extern "C" {

/* ---- ray queries ---- */
// Both entry points read the scene bound to kernel 0 as it is now: a stale scene is prepared first (after the deferred frames that read
// the old one), as do_dispatch does; otherwise the deferred batch stays deferred — a query only reads the scene.  The query is enqueued
// on the context's stream WITHOUT marking it touched (the frame loop's overlap bookkeeping, counters and launches are not affected).
static int query_prepare(urt_context* ctx, const void* rays, int n, const void* out, int flags) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (n < 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "ray query: negative ray count");
  if (flags != URT_QUERY_CLOSEST && flags != URT_QUERY_ANY) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "ray query: unknown flags");
  if (n > 0 && (!rays || !out)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "ray query: rays / out is NULL");
  if (n == 0) return URT_OK;
  URT_HIP(ctx, hipSetDevice(ctx->device));
  return current_scene(ctx);
}

int urt_ray_query(urt_context* ctx, const urt_Ray* rays, int n, void* out, int flags) {
  URT_GUARD_BEGIN
  int rc = query_prepare(ctx, rays, n, out, flags);
  if (rc || n == 0) return rc;
  // the wait for the stream at growth is new here and costs nothing: no query still reads the old pair, as this form synchronises the
  // same stream before it returns; device-form queries the caller enqueued since are ordered like everything else on it
  if (int r = reserve(ctx, ctx->q_rays, (size_t)n, "ray query: scratch allocation", ctx->stream)) return r;
  if (int r = reserve(ctx, ctx->q_out, (size_t)n, "ray query: scratch allocation", ctx->stream)) return r;
  const size_t out_bytes = (size_t)n * (flags == URT_QUERY_ANY ? sizeof(int32_t) : sizeof(urt_RayHit));
  URT_HIP(ctx, hipMemcpyAsync(ctx->q_rays.get(), rays, (size_t)n * sizeof(urt_Ray), hipMemcpyHostToDevice, ctx->stream));
  URT_HIP(ctx, launch_query(ctx->scene.ds, lane_stack_size(ctx), (const float4*)ctx->q_rays.get(), n, ctx->q_out.get(), flags == URT_QUERY_ANY, ctx->stream));
  URT_HIP(ctx, hipMemcpyAsync(out, ctx->q_out.get(), out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  URT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return check_watchdog(ctx);
  URT_GUARD_END(ctx)
}

int urt_ray_query_device(urt_context* ctx, const void* d_rays, int n, void* d_out, int flags) {
  URT_GUARD_BEGIN
  int rc = query_prepare(ctx, d_rays, n, d_out, flags);
  if (rc || n == 0) return rc;
  if (((uintptr_t)d_rays & 15u) || ((uintptr_t)d_out & (flags == URT_QUERY_ANY ? 3u : 15u)))
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "ray query: d_rays must be 16-byte aligned, d_out 16-byte (closest hit) / 4-byte (any hit) aligned");
  URT_HIP(ctx, launch_query(ctx->scene.ds, lane_stack_size(ctx), (const float4*)d_rays, n, d_out, flags == URT_QUERY_ANY, ctx->stream));
  return URT_OK;
  URT_GUARD_END(ctx)
}

/* ---- radiance queries ---- */
// Scene, ordering and counters as the ray queries: enqueued on the context's stream WITHOUT marking it touched.  Unlike them the kernel
// reads the sky, so deferred work that writes the texture bound as _SkyboxTexture is submitted first.  Everything is checked before
// anything is enqueued; on success *launch holds the batch but for its pointers.
static int radiance_prepare(urt_context* ctx, const void* in, int n, int samples, int bounces, const void* out, int flags, bool host,
                            DevScene* S, FrameUniforms* C, RadianceBatch* launch) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (n < 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "radiance query: negative query count");
  if (flags != URT_RADIANCE_RAYS && flags != URT_RADIANCE_PIXELS) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "radiance query: unknown flags");
  if (samples < 1 || samples > 4096) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "radiance query: samples must be 1..4096");
  if (bounces < 0 || bounces > 64) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "radiance query: bounces must be 0..64");
  if (n > 0 && (!in || !out)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "radiance query: in / out is NULL");
  if (n == 0) return URT_OK;
  const bool pixels = flags == URT_RADIANCE_PIXELS;
  *C = pixels ? bound_camera(ctx) : FrameUniforms{};
  int width = 0, height = 0;
  if (pixels) {
    const Texture* res = find_texture(ctx, ctx->t_result);
    if (!res) return fail(ctx, URT_ERR_UNBOUND, "radiance query: no texture bound to \"Result\"");
    if (!ctx->c2w_set || !ctx->invp_set)
      return fail(ctx, URT_ERR_UNBOUND, "radiance query: _CameraToWorld / _CameraInverseProjection not set");
    width = res->w; height = res->h;
    if (host) {
      const urt_PathPixel* p = (const urt_PathPixel*)in;
      for (int i = 0; i < n; i++)
        if (p[i].x < 0 || p[i].x >= res->w || p[i].y < 0 || p[i].y >= res->h)
          return fail(ctx, URT_ERR_INVALID_ARGUMENT, "radiance query: pixel " + std::to_string(i) + " lies outside the texture bound as Result");
    }
  }
  if (!host && (((uintptr_t)in & (pixels ? 7u : 15u)) || ((uintptr_t)out & 15u)))
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "radiance query: device rays and output must be 16-byte aligned, pixels 8-byte aligned");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  const urt_context::Pending& B = ctx->pend;
  bool sky_written = false;                                  // (the deferring calls keep such work out of a batch; a texture bound as the sky afterwards is not covered by that)
  if (B.n > 0 && ctx->t_sky) {
    sky_written = B.tex == ctx->t_sky;
    for (const PostOp& q : B.ops) sky_written = sky_written || q.dst == ctx->t_sky || q.count == ctx->t_sky;
  }
  if (ctx->scene_dirty || sky_written) { int rc = flush_pending(ctx); if (rc) return rc; }   // the deferred frames read the scene that is about to be replaced
  if (ctx->scene_dirty) { int rc = prepare_scene(ctx); if (rc) return rc; }
  *S = ctx->scene.ds;
  { int rc = bind_sky(ctx, *S); if (rc) return rc; }
  *launch = RadianceBatch{};
  launch->n = n; launch->samples = samples; launch->bounces = bounces; launch->pixels = pixels; launch->width = width; launch->height = height;
  const bool persist = ctx->opt.radiance_persist < 0 ? kRadiancePersistAuto : ctx->opt.radiance_persist != 0;
  if (persist) {
    if (!ctx->rq_next) URT_HIP(ctx, ctx->rq_next.alloc(1));
    launch->work_counter = ctx->rq_next.get(); launch->n_cus = ctx->n_cus;
  }
  return URT_OK;
}

int urt_radiance_query(urt_context* ctx, const void* in, int n, int samples, int bounces, float* out_rgba, int flags) {
  URT_GUARD_BEGIN
  DevScene S; FrameUniforms C; RadianceBatch B;
  int rc = radiance_prepare(ctx, in, n, samples, bounces, out_rgba, flags, true, &S, &C, &B);
  if (rc || n == 0) return rc;
  const size_t in_bytes = (size_t)n * (B.pixels ? sizeof(urt_PathPixel) : sizeof(urt_PathRay));
  if (int r = reserve(ctx, ctx->rq_in, in_bytes, "radiance query: scratch allocation", ctx->stream)) return r;
  if (int r = reserve(ctx, ctx->rq_out, (size_t)n, "radiance query: scratch allocation", ctx->stream)) return r;
  B.in = ctx->rq_in.get(); B.out = ctx->rq_out.get();
  URT_HIP(ctx, hipMemcpyAsync(ctx->rq_in.get(), in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  URT_HIP(ctx, launch_radiance(S, lane_stack_size(ctx), C, B, ctx->stream));
  URT_HIP(ctx, hipMemcpyAsync(out_rgba, ctx->rq_out.get(), (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  URT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return check_watchdog(ctx);
  URT_GUARD_END(ctx)
}

int urt_radiance_query_device(urt_context* ctx, const void* d_in, int n, int samples, int bounces, void* d_out_rgba, int flags) {
  URT_GUARD_BEGIN
  DevScene S; FrameUniforms C; RadianceBatch B;
  int rc = radiance_prepare(ctx, d_in, n, samples, bounces, d_out_rgba, flags, false, &S, &C, &B);
  if (rc || n == 0) return rc;
  B.in = d_in; B.out = (float4*)d_out_rgba;
  URT_HIP(ctx, launch_radiance(S, lane_stack_size(ctx), C, B, ctx->stream));
  return URT_OK;
  URT_GUARD_END(ctx)
}

/* ---- feature buffers ---- */
// Everything else that could observe the images flushes first: the deferred frames are submitted, then a stale scene is prepared, then
// the kernel is enqueued on the main stream (marked touched, as urt_texture_set_pixels does).  Every argument is checked before anything
// is submitted or written.  The counters are not changed.
int urt_render_aov(urt_context* ctx, urt_handle hit, urt_handle normal, urt_handle albedo, urt_handle id, int flags) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  if (flags != URT_AOV_PIXEL_CENTER && flags != URT_AOV_FRAME_RAY) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "render_aov: unknown flags");
  const TexArg a[4] = {{hit, nullptr, true}, {normal, nullptr, true}, {albedo, nullptr, true}, {id, nullptr, true}};
  Texture* t[4];
  int width = 0, height = 0, n = 0;
  if (int rc = resolve_textures(ctx, "render_aov", a, 4, t, "a texture is given for two targets")) return rc;
  for (int k = 0; k < 4; k++) {
    if (!t[k]) continue;
    if (a[k].h == ctx->t_sky) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "render_aov: a target is the texture bound as _SkyboxTexture");
    if (n++ == 0) { width = t[k]->w; height = t[k]->h; }
    else if (t[k]->w != width || t[k]->h != height) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "render_aov: the targets differ in size");
  }
  if (n == 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "render_aov: no target given");
  if (int rc = check_height(ctx, "render_aov", "targets", height)) return rc;
  if (!ctx->c2w_set || !ctx->invp_set)
    return fail(ctx, URT_ERR_UNBOUND, "render_aov: _CameraToWorld / _CameraInverseProjection not set");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  { int rc = flush_pending(ctx); if (rc) return rc; }
  if (ctx->scene_dirty) { int rc = prepare_scene(ctx); if (rc) return rc; }
  DevScene S = ctx->scene.ds;
  { int rc = bind_sky(ctx, S); if (rc) return rc; }
  AovTargets T{};
  T.hit = t[0] ? t[0]->dev : nullptr; T.normal = t[1] ? t[1]->dev : nullptr;
  T.albedo = t[2] ? t[2]->dev : nullptr; T.id = t[3] ? t[3]->dev : nullptr;
  T.width = width; T.height = height;
  for (int k = 0; k < 4; k++) if (t[k]) t[k]->other_writes = true;
  URT_HIP(ctx, launch_aov(S, ctx->scene.aov_albedo, lane_stack_size(ctx), bound_camera(ctx), flags == URT_AOV_FRAME_RAY, T, touch(ctx)));
  return URT_OK;
  URT_GUARD_END(ctx)
}

/* ---- denoising ---- */
// Every argument is checked and the scratch is grown before anything is submitted: on an error nothing is enqueued.  Then the deferred
// frames are submitted (src is usually a deferred blit's destination) and the passes are enqueued on the main stream.  The scene is not
// read and the counters are not changed.
int urt_denoise(urt_context* ctx, urt_handle src, urt_handle dst, urt_handle hit, urt_handle normal, urt_handle albedo,
                const urt_DenoiseParams* params) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  urt_DenoiseParams P{URT_DENOISE_DEFAULT_ITERATIONS, URT_DENOISE_DEFAULT_SIGMA_COLOR, URT_DENOISE_DEFAULT_SIGMA_NORMAL,
                      URT_DENOISE_DEFAULT_SIGMA_DEPTH};
  if (params) P = *params;
  if (P.iterations < 1 || P.iterations > 5) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "denoise: iterations must be 1..5");
  if (std::isnan(P.sigma_color) || std::isnan(P.sigma_normal) || std::isnan(P.sigma_depth))
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "denoise: a sigma is NaN");
  const TexArg a[5] = {{src, "src", false}, {dst, "dst", false}, {hit, "hit", false}, {normal, "normal", false},
                       {albedo, "albedo", true}};                  // no albedo: no demodulation
  Texture* t[5];
  if (int rc = resolve_textures(ctx, "denoise", a, 5, t)) return rc;
  if (dst == hit || dst == normal || dst == albedo)
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "denoise: dst is one of the guide textures");
  if (dst == ctx->t_sky) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "denoise: dst is the texture bound as _SkyboxTexture");
  const int width = t[0]->w, height = t[0]->h;
  if (int rc = check_same_size(ctx, "denoise", t, 5)) return rc;
  if (int rc = check_height(ctx, "denoise", "textures", height)) return rc;
  URT_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)width * (size_t)height;
  if (int rc = reserve(ctx, ctx->dn_scratch, 3 * n, "denoise: scratch allocation", ctx->stream)) return rc;
  { int rc = flush_pending(ctx); if (rc) return rc; }
  DenoiseImages I{};                                               // device pointers after the flush (a Result texture may be renamed)
  I.src = t[0]->dev; I.dst = t[1]->dev; I.hit = t[2]->dev; I.normal = t[3]->dev; I.albedo = t[4] ? t[4]->dev : nullptr;
  I.scratch = ctx->dn_scratch.get(); I.width = width; I.height = height;
  DenoiseSettings S{P.iterations, P.sigma_color, P.sigma_normal, P.sigma_depth};
  t[1]->other_writes = true;
  URT_HIP(ctx, launch_denoise(I, S, touch(ctx)));
  return URT_OK;
  URT_GUARD_END(ctx)
}

/* ---- temporal reprojection ---- */
// Every argument is checked before anything is submitted: on an error nothing is enqueued.  Then the deferred frames are submitted
// (prev_color is usually a deferred blend's destination) and k_reproject is enqueued on the main stream.  The scene is not read and the
// counters are not changed.  with_motion: urt_reproject_objects, whose tables (ComputeBuffers: host copies) are uploaded on the same
// stream in front of k_reproject_objects; without a table given the call is urt_reproject's, kernel included.  deform (only with
// with_motion): urt_reproject_deformed, whose four buffers are read through their device mirrors; without one the call is
// urt_reproject_objects', kernel included.
static int reproject_impl(urt_context* ctx, const urt_ReprojectImages* images, const urt_ReprojectParams* params,
                          const urt_ReprojectMotion* motion, bool with_motion, const urt_ReprojectDeform* deform = nullptr) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!images || !params) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "reproject: images or params is NULL");
  URT_GUARD_BEGIN
  const urt_ReprojectParams P = *params;
  urt_ReprojectMotion Mo{};
  if (with_motion && motion) Mo = *motion;
  Buffer* tab[2] = {nullptr, nullptr};
  if (with_motion) {
    if (Mo.flags != 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "reproject: motion flags must be 0");
    if (!valid_max_history(Mo.moved_max_history)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "reproject: moved_max_history must be 0 or >= 1");
    const urt_handle th[2] = {Mo.mesh_motion, Mo.sphere_motion};
    for (int k = 0; k < 2; k++) {
      if (!th[k]) continue;
      auto it = ctx->buffers.find(th[k]);
      if (it == ctx->buffers.end())
        return fail(ctx, URT_ERR_INVALID_HANDLE, std::string("reproject: unknown ") + (k ? "sphere_motion" : "mesh_motion") + " buffer handle");
      if (it->second.stride != (int)sizeof(urt_ObjectMotion))
        return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string("reproject: the stride of ") + (k ? "sphere_motion" : "mesh_motion") + " is not 48");
      tab[k] = &it->second;
    }
  }
  enum { kPrevVertices, kIndices, kPrevObjects, kDeformed, kDeformBuffers };
  Buffer* db[kDeformBuffers] = {nullptr, nullptr, nullptr, nullptr};
  urt_ReprojectDeform De{};
  if (deform) {
    De = *deform;
    if (De.flags != 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "reproject: deform flags must be 0");
    if (std::isnan(De.normal_threshold)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "reproject: the deform normal_threshold is NaN");
    const BufArg da[kDeformBuffers] = {{De.prev_vertices, "prev_vertices", URT_STRIDE_VEC3}, {De.indices, "indices", URT_STRIDE_INDEX},
                                       {De.prev_mesh_objects, "prev_mesh_objects", URT_STRIDE_MESHOBJECT}, {De.deformed, "deformed", 4}};
    for (int k = 0; k < kDeformBuffers; k++)                 // one by one: a buffer's stride is checked before the next handle is looked up
      if (int rc = resolve_buffers(ctx, "reproject", &da[k], 1, &db[k])) return rc;
    if (db[kIndices]->count % 3 != 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "reproject: the count of indices is not a multiple of 3");
    if (db[kDeformed]->count != db[kPrevObjects]->count)
      return fail(ctx, URT_ERR_INVALID_ARGUMENT, "reproject: the counts of deformed and prev_mesh_objects differ");
  }
  if (P.flags != 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "reproject: flags must be 0");
  if (std::isnan(P.normal_threshold) || std::isnan(P.plane_threshold)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "reproject: a threshold is NaN");
  if (!valid_max_history(P.max_history)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "reproject: max_history must be 0 or >= 1");
  enum { kInputs = 8, kImages = 11 };
  const TexArg a[kImages] = {{images->prev_color, "prev_color", false}, {images->prev_count, "prev_count", false}, {images->prev_hit, "prev_hit", false},
                             {images->prev_normal, "prev_normal", false}, {images->prev_id, "prev_id", false}, {images->hit, "hit", false},
                             {images->normal, "normal", false}, {images->id, "id", false}, {images->color, "color", false},
                             {images->count, "count", false}, {images->motion, "motion", true}};   // no motion image wanted: 0
  Texture* t[kImages];
  if (int rc = resolve_textures(ctx, "reproject", a, kImages, t)) return rc;
  const int width = t[0]->w, height = t[0]->h;
  if (int rc = check_same_size(ctx, "reproject", t, kImages)) return rc;
  if (int rc = check_outputs(ctx, "reproject", a, kInputs, kImages)) return rc;
  if (int rc = check_height(ctx, "reproject", "textures", height)) return rc;
  if (!ctx->c2w_set || !ctx->invp_set)
    return fail(ctx, URT_ERR_UNBOUND, "reproject: _CameraToWorld / _CameraInverseProjection never set (SetMatrix, RM:774-775)");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = mirror_buffers(ctx, db, kDeformBuffers)) return rc;   // (before anything is enqueued: an allocation can fail)
  { int rc = flush_pending(ctx); if (rc) return rc; }
  ReprojectImages I{};                                             // device pointers after the flush (a Result texture may be renamed)
  I.prev_color = t[0]->dev; I.prev_count = t[1]->dev; I.prev_hit = t[2]->dev; I.prev_normal = t[3]->dev; I.prev_id = t[4]->dev;
  I.hit = t[5]->dev; I.normal = t[6]->dev; I.id = t[7]->dev;
  I.color = t[8]->dev; I.count = t[9]->dev; I.motion = t[10] ? t[10]->dev : nullptr;
  I.width = width; I.height = height;
  ReprojectSettings S{};
  std::memcpy(S.m, P.prev_world_to_clip, sizeof S.m);
  std::memcpy(S.c2w, ctx->c2w, sizeof S.c2w);
  std::memcpy(S.invp, ctx->invp, sizeof S.invp);
  S.max_history = P.max_history; S.normal_threshold = P.normal_threshold; S.plane_threshold = P.plane_threshold;
  if (tab[0] || tab[1] || deform) {
    ReprojectMotion T{};
    for (int k = 0; k < 2; k++) {
      if (!tab[k]) continue;
      const size_t bytes = (size_t)tab[k]->count * sizeof(urt_ObjectMotion);
      if (int rc = buffer_sync_host(ctx, *tab[k])) return rc;                    // a table written on the device
      if (int rc = reserve(ctx, ctx->mo_table[k], (size_t)tab[k]->count, "reproject: motion table allocation", ctx->stream)) return rc;
      URT_HIP(ctx, hipMemcpyAsync(ctx->mo_table[k].get(), tab[k]->host.data(), bytes, hipMemcpyHostToDevice, touch(ctx)));
    }
    T.mesh = tab[0] ? (const float4*)ctx->mo_table[0].get() : nullptr; T.n_mesh = tab[0] ? tab[0]->count : 0;
    T.sphere = tab[1] ? (const float4*)ctx->mo_table[1].get() : nullptr; T.n_sphere = tab[1] ? tab[1]->count : 0;
    T.moved_max_history = Mo.moved_max_history;
    for (int k = kInputs; k < kImages; k++) if (t[k]) t[k]->other_writes = true;
    if (deform) {
      ReprojectDeform D{};
      D.vertices = (const float*)db[kPrevVertices]->mirror.get(); D.n_vertices = db[kPrevVertices]->count;
      D.indices = (const int*)db[kIndices]->mirror.get(); D.n_indices = db[kIndices]->count;
      D.objects = (const float4*)db[kPrevObjects]->mirror.get(); D.flags = (const int*)db[kDeformed]->mirror.get();
      D.n_objects = db[kDeformed]->count;
      D.normal_threshold = De.normal_threshold;
      URT_HIP(ctx, launch_reproject_deformed(I, S, T, D, touch(ctx)));
      return URT_OK;
    }
    URT_HIP(ctx, launch_reproject_objects(I, S, T, touch(ctx)));
    return URT_OK;
  }
  for (int k = kInputs; k < kImages; k++) if (t[k]) t[k]->other_writes = true;
  URT_HIP(ctx, launch_reproject(I, S, touch(ctx)));
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_reproject(urt_context* ctx, const urt_ReprojectImages* images, const urt_ReprojectParams* params) {
  return reproject_impl(ctx, images, params, nullptr, false);
}

int urt_reproject_objects(urt_context* ctx, const urt_ReprojectImages* images, const urt_ReprojectParams* params,
                          const urt_ReprojectMotion* motion) {
  return reproject_impl(ctx, images, params, motion, true);
}

int urt_reproject_deformed(urt_context* ctx, const urt_ReprojectImages* images, const urt_ReprojectParams* params,
                           const urt_ReprojectMotion* motion, const urt_ReprojectDeform* deform) {
  return reproject_impl(ctx, images, params, motion, true, deform);
}

/* ---- guide-driven upsampling ---- */
// As urt_reproject: every argument is checked before anything is submitted, then the deferred frames are submitted (low_color is usually
// a deferred blend's destination) and k_upsample is enqueued on the main stream.  The scene is not read and the counters are not
// changed.  The one image call with textures of two sizes: the low_* images share one, the others another.
int urt_upsample(urt_context* ctx, const urt_UpsampleImages* images, const urt_UpsampleParams* params) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!images) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "upsample: images is NULL");
  URT_GUARD_BEGIN
  urt_UpsampleParams P{URT_UPSAMPLE_DEFAULT_NORMAL_THRESHOLD, URT_UPSAMPLE_DEFAULT_PLANE_THRESHOLD, URT_UPSAMPLE_DEFAULT_COUNT_SCALE,
                       URT_UPSAMPLE_DEFAULT_FLAGS};
  if (params) P = *params;
  if (P.flags & ~(URT_UPSAMPLE_WIDE_FALLBACK | URT_UPSAMPLE_SKY_FROM_ALBEDO)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "upsample: unknown flags");
  if (std::isnan(P.normal_threshold) || std::isnan(P.plane_threshold)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "upsample: a threshold is NaN");
  if (!std::isfinite(P.count_scale) || !(P.count_scale > 0.0f)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "upsample: count_scale must be finite and > 0");
  enum { kLow = 5, kInputs = 9, kImages = 11 };                    // the low grid's images, then the full grid's; the outputs last
  const TexArg a[kImages] = {{images->low_color, "low_color", false}, {images->low_count, "low_count", true}, {images->low_hit, "low_hit", false},
                             {images->low_normal, "low_normal", false}, {images->low_id, "low_id", false}, {images->hit, "hit", false},
                             {images->normal, "normal", false}, {images->id, "id", false}, {images->albedo, "albedo", true},
                             {images->color, "color", false}, {images->count, "count", true}};
  Texture* t[kImages];
  if (int rc = resolve_textures(ctx, "upsample", a, kImages, t)) return rc;
  if (int rc = check_same_size(ctx, "upsample (low grid)", t, kLow)) return rc;
  if (int rc = check_same_size(ctx, "upsample (full grid)", t + kLow, kImages - kLow)) return rc;
  if (int rc = check_outputs(ctx, "upsample", a, kInputs, kImages)) return rc;
  if (int rc = check_height(ctx, "upsample", "full-grid textures", t[kLow]->h)) return rc;
  URT_HIP(ctx, hipSetDevice(ctx->device));
  { int rc = flush_pending(ctx); if (rc) return rc; }
  UpsampleImages I{};                                              // device pointers after the flush (a Result texture may be renamed)
  I.low_color = t[0]->dev; I.low_count = t[1] ? t[1]->dev : nullptr; I.low_hit = t[2]->dev; I.low_normal = t[3]->dev; I.low_id = t[4]->dev;
  I.hit = t[5]->dev; I.normal = t[6]->dev; I.id = t[7]->dev; I.albedo = t[8] ? t[8]->dev : nullptr;
  I.color = t[9]->dev; I.count = t[10] ? t[10]->dev : nullptr;
  I.low_width = t[0]->w; I.low_height = t[0]->h; I.width = t[kLow]->w; I.height = t[kLow]->h;
  const UpsampleSettings S{P.normal_threshold, P.plane_threshold, P.count_scale, (P.flags & URT_UPSAMPLE_WIDE_FALLBACK) != 0,
                           (P.flags & URT_UPSAMPLE_SKY_FROM_ALBEDO) != 0};
  for (int k = kInputs; k < kImages; k++) if (t[k]) t[k]->other_writes = true;
  URT_HIP(ctx, launch_upsample(I, S, touch(ctx)));
  return URT_OK;
  URT_GUARD_END(ctx)
}

/* ---- auto-exposure and tone mapping ---- */
// As urt_reproject: every argument is checked before anything is submitted, then the deferred frames are submitted (src is usually a
// deferred blend's destination) and the kernels of csrc/tonemap.hip are enqueued on the main stream.  The scene is not read and the
// counters are not changed.  The exposure state is the caller's device memory: the library keeps nothing between the calls.
int urt_auto_exposure(urt_context* ctx, urt_handle src, urt_handle count, const urt_ExposureParams* params, void* d_state) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  urt_ExposureParams P{URT_EXPOSURE_DEFAULT_KEY, URT_EXPOSURE_DEFAULT_MIN_EXPOSURE, URT_EXPOSURE_DEFAULT_MAX_EXPOSURE,
                       URT_EXPOSURE_DEFAULT_RATE, URT_EXPOSURE_DEFAULT_LOW_PERMILLE, URT_EXPOSURE_DEFAULT_HIGH_PERMILLE};
  if (params) P = *params;
  if (!d_state || ((uintptr_t)d_state & 15u)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "auto_exposure: d_state must be 16-byte aligned device memory");
  for (const float v : {P.key, P.min_exposure, P.max_exposure})
    if (!std::isfinite(v) || !(v > 0.0f))
      return fail(ctx, URT_ERR_INVALID_ARGUMENT, "auto_exposure: key, min_exposure and max_exposure must be finite and > 0");
  if (P.min_exposure > P.max_exposure) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "auto_exposure: min_exposure is above max_exposure");
  if (!(P.rate > 0.0f)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "auto_exposure: rate must be > 0");
  if (!(0 <= P.low_permille && P.low_permille < P.high_permille && P.high_permille <= 1000))
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "auto_exposure: the permilles must satisfy 0 <= low < high <= 1000");
  const TexArg a[2] = {{src, "src", false}, {count, "count", true}};
  Texture* t[2];
  if (int rc = resolve_textures(ctx, "auto_exposure", a, 2, t)) return rc;
  if (int rc = check_same_size(ctx, "auto_exposure", t, 2)) return rc;
  const size_t n_texels = (size_t)t[0]->w * (size_t)t[0]->h;
  if (n_texels > 0x7fffffffull) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "auto_exposure: src has more than 2^31 - 1 texels");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->ex_accum) {                                            // the histogram's accumulators: zeroed once, here; every call leaves them zero
    const size_t words = (size_t)kExposureCopies * (size_t)kExposureWords;
    if (int rc = reserve(ctx, ctx->ex_accum, words, "auto_exposure: scratch allocation", ctx->stream)) return rc;
    URT_HIP(ctx, hipMemsetAsync(ctx->ex_accum.get(), 0, words * sizeof(unsigned int), ctx->stream));
    URT_HIP(ctx, hipStreamSynchronize(ctx->stream));               // (the first call only: whatever stream a later call is issued on finds them zero)
  }
  { int rc = flush_pending(ctx); if (rc) return rc; }
  const ExposureSettings S{P.key, P.min_exposure, P.max_exposure, P.rate, P.low_permille, P.high_permille};
  URT_HIP(ctx, launch_auto_exposure(t[0]->dev, t[1] ? t[1]->dev : nullptr, n_texels, S, ctx->ex_accum.get(), (ExposureState*)d_state,
                                    touch(ctx)));                  // device pointers after the flush (a Result texture may be renamed)
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_tonemap(urt_context* ctx, urt_handle src, urt_handle dst, const urt_TonemapParams* params, const void* d_state) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  urt_TonemapParams P{URT_TONEMAP_DEFAULT_EXPOSURE, URT_TONEMAP_DEFAULT_WHITE, URT_TONEMAP_DEFAULT_OP, URT_TONEMAP_DEFAULT_FLAGS};
  if (params) P = *params;
  if (P.op != URT_TONEMAP_LINEAR && P.op != URT_TONEMAP_REINHARD && P.op != URT_TONEMAP_ACES)
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "tonemap: unknown op");
  if (P.flags != 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "tonemap: flags must be 0");
  if (!std::isfinite(P.exposure) || !(P.exposure > 0.0f)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "tonemap: exposure must be finite and > 0");
  if (!(P.white >= 0.01f && P.white <= 65504.0f)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "tonemap: white must lie in [0.01, 65504]");
  if ((uintptr_t)d_state & 15u) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "tonemap: d_state must be 16-byte aligned");
  const TexArg a[2] = {{src, "src", false}, {dst, "dst", false}};
  Texture* t[2];
  if (int rc = resolve_textures(ctx, "tonemap", a, 2, t)) return rc;
  if (int rc = check_same_size(ctx, "tonemap", t, 2)) return rc;
  if (dst == ctx->t_sky) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "tonemap: dst is the texture bound as _SkyboxTexture");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  { int rc = flush_pending(ctx); if (rc) return rc; }
  const TonemapSettings S{P.exposure, P.white, P.op};
  t[1]->other_writes = true;
  URT_HIP(ctx, launch_tonemap(t[0]->dev, t[1]->dev, (size_t)t[0]->w * (size_t)t[0]->h, S, (const ExposureState*)d_state, touch(ctx)));
  return URT_OK;
  URT_GUARD_END(ctx)
}

/* ---- depth of field ---- */
// As urt_bloom: every argument is checked before anything is allocated or submitted, then the scratch is grown, the deferred frames are
// submitted and the kernels of csrc/dof.hip are enqueued on the main stream.  The scene is not read and the counters are not changed.
int urt_depth_of_field(urt_context* ctx, urt_handle src, urt_handle hit, urt_handle dst, const urt_DofParams* params) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  urt_DofParams P{URT_DOF_DEFAULT_FOCUS_DISTANCE, URT_DOF_DEFAULT_SCALE, URT_DOF_DEFAULT_MAX_RADIUS, URT_DOF_DEFAULT_FLAGS};
  if (params) P = *params;
  if (!std::isfinite(P.focus_distance) || !(P.focus_distance > 0.0f))
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "depth_of_field: focus_distance must be finite and > 0");
  if (!std::isfinite(P.scale) || !(P.scale >= 0.0f)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "depth_of_field: scale must be finite and >= 0");
  if (!(P.max_radius >= 0.5f && P.max_radius <= URT_DOF_MAX_RADIUS))
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "depth_of_field: max_radius must lie in [0.5, 16]");
  if (P.flags & ~URT_DOF_FLAG_COC) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "depth_of_field: unknown flag bits");
  const TexArg a[3] = {{src, "src", false}, {hit, "hit", false}, {dst, "dst", false}};
  Texture* t[3];
  if (int rc = resolve_textures(ctx, "depth_of_field", a, 3, t)) return rc;
  if (int rc = check_same_size(ctx, "depth_of_field", t, 3)) return rc;
  if (int rc = check_outputs(ctx, "depth_of_field", a, 2, 3)) return rc;      // dst is neither src nor hit (no in-place form) nor the sky
  const int width = t[0]->w, height = t[0]->h;
  if (int rc = check_height(ctx, "depth_of_field", "textures", height)) return rc;
  if (width > kDofMaxExtent) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "depth_of_field: textures wider than 2^30 pixels");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = reserve(ctx, ctx->df_scratch, dof_scratch_floats(width, height), "depth_of_field: scratch allocation", ctx->stream)) return rc;
  { int rc = flush_pending(ctx); if (rc) return rc; }
  const DofSettings S{P.focus_distance, P.scale, P.max_radius, P.flags};
  t[2]->other_writes = true;
  URT_HIP(ctx, launch_depth_of_field(t[0]->dev, t[1]->dev, t[2]->dev, width, height, S, ctx->df_scratch.get(), touch(ctx)));
                                                                   // (device pointers after the flush: a Result texture may be renamed)
  return URT_OK;
  URT_GUARD_END(ctx)
}

/* ---- motion blur ---- */
// As urt_depth_of_field: every argument is checked before anything is allocated or submitted, then the scratch is grown, the deferred
// frames are submitted and the kernels of csrc/motion_blur.hip are enqueued on the main stream.  The scene is not read and the counters
// are not changed.
int urt_motion_blur(urt_context* ctx, urt_handle src, urt_handle motion, urt_handle hit, urt_handle dst, const urt_MotionBlurParams* params) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  urt_MotionBlurParams P{URT_MOTION_BLUR_DEFAULT_SHUTTER, URT_MOTION_BLUR_DEFAULT_MAX_RADIUS, 0, 0};
  if (params) P = *params;
  if (!(P.shutter >= 0.0f && P.shutter <= 1.0f)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "motion_blur: shutter must lie in [0, 1]");
  if (!(P.max_radius >= 0.5f && P.max_radius <= URT_MOTION_BLUR_MAX_RADIUS))
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "motion_blur: max_radius must lie in [0.5, 16]");
  if (P.flags & ~URT_MOTION_BLUR_FLAG_VELOCITY) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "motion_blur: unknown flag bits");
  if (P.reserved != 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "motion_blur: reserved must be 0");
  const TexArg a[4] = {{src, "src", false}, {motion, "motion", false}, {hit, "hit", false}, {dst, "dst", false}};
  Texture* t[4];
  if (int rc = resolve_textures(ctx, "motion_blur", a, 4, t)) return rc;
  if (int rc = check_same_size(ctx, "motion_blur", t, 4)) return rc;
  if (int rc = check_outputs(ctx, "motion_blur", a, 3, 4)) return rc;         // dst is none of the inputs (no in-place form) nor the sky
  const int width = t[0]->w, height = t[0]->h;
  if (int rc = check_height(ctx, "motion_blur", "textures", height)) return rc;
  if (width > kMotionBlurMaxExtent) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "motion_blur: textures wider than 2^30 pixels");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = reserve(ctx, ctx->mb_scratch, motion_blur_scratch_floats(width, height), "motion_blur: scratch allocation", ctx->stream)) return rc;
  { int rc = flush_pending(ctx); if (rc) return rc; }
  const MotionBlurSettings S{P.shutter, P.max_radius, P.flags};
  t[3]->other_writes = true;
  URT_HIP(ctx, launch_motion_blur(t[0]->dev, t[1]->dev, t[2]->dev, t[3]->dev, width, height, S, ctx->mb_scratch.get(), touch(ctx)));
                                                                   // (device pointers after the flush: a Result texture may be renamed)
  return URT_OK;
  URT_GUARD_END(ctx)
}

/* ---- bloom ---- */
// As urt_tonemap: every argument is checked before anything is allocated or submitted, then the pyramid's scratch is grown, the deferred
// frames are submitted and the kernels of csrc/bloom.hip are enqueued on the main stream.  The scene is not read and the counters are not
// changed.
int urt_bloom(urt_context* ctx, urt_handle src, urt_handle dst, const urt_BloomParams* params, const void* d_state) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  urt_BloomParams P{URT_BLOOM_DEFAULT_THRESHOLD, URT_BLOOM_DEFAULT_SOFT_KNEE, URT_BLOOM_DEFAULT_CLAMP, URT_BLOOM_DEFAULT_SCATTER,
                    URT_BLOOM_DEFAULT_INTENSITY, URT_BLOOM_DEFAULT_LEVELS, URT_BLOOM_DEFAULT_FLAGS};
  if (params) P = *params;
  if (!(P.threshold >= 0.0f && P.threshold <= 65504.0f)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "bloom: threshold must lie in [0, 65504]");
  if (!(P.soft_knee >= 0.0f && P.soft_knee <= 1.0f)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "bloom: soft_knee must lie in [0, 1]");
  if (!(P.clamp > 0.0f && P.clamp <= 65504.0f)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "bloom: clamp must lie in (0, 65504]");
  if (!(P.scatter >= 0.0f && P.scatter <= 1.0f)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "bloom: scatter must lie in [0, 1]");
  if (!std::isfinite(P.intensity) || !(P.intensity >= 0.0f)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "bloom: intensity must be finite and >= 0");
  if (P.levels < 1 || P.levels > kBloomMaxLevels) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "bloom: levels must be 1..16");
  if (P.flags & ~URT_BLOOM_FLAG_ONLY) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "bloom: unknown flag bits");
  if ((uintptr_t)d_state & 15u) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "bloom: d_state must be 16-byte aligned");
  const TexArg a[2] = {{src, "src", false}, {dst, "dst", false}};
  Texture* t[2];
  if (int rc = resolve_textures(ctx, "bloom", a, 2, t)) return rc;
  if (int rc = check_same_size(ctx, "bloom", t, 2)) return rc;
  if (dst == ctx->t_sky) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "bloom: dst is the texture bound as _SkyboxTexture");
  const int width = t[0]->w, height = t[0]->h;
  if (int rc = check_height(ctx, "bloom", "textures", height)) return rc;
  if (width > kBloomMaxExtent) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "bloom: textures wider than 2^30 pixels");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = reserve(ctx, ctx->bl_pyramid, bloom_levels(width, height, P.levels).texels, "bloom: scratch allocation", ctx->stream)) return rc;
  { int rc = flush_pending(ctx); if (rc) return rc; }
  const BloomSettings S{P.threshold, P.soft_knee, P.clamp, P.scatter, P.intensity, P.levels, P.flags};
  t[1]->other_writes = true;
  URT_HIP(ctx, launch_bloom(t[0]->dev, t[1]->dev, width, height, S, (const ExposureState*)d_state, ctx->bl_pyramid.get(), touch(ctx)));
                                                                   // (device pointers after the flush: a Result texture may be renamed)
  return URT_OK;
  URT_GUARD_END(ctx)
}

/* ---- resampling ---- */
// urt_select_pixels observes the count texture: every argument is checked and the scratch is grown first, then the deferred frames are
// submitted, the three phases of csrc/resample.hip are enqueued on the main stream and the call waits once, for the total.  The scene is
// not read and the counters are not changed.
int urt_select_pixels(urt_context* ctx, urt_handle count, float below, void* d_pixels, int capacity, int* out_n) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  if (!out_n) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "select_pixels: out_n is NULL");
  if (std::isnan(below)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "select_pixels: below is NaN");
  if (capacity < 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "select_pixels: negative capacity");
  if (capacity > 0 && !d_pixels) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "select_pixels: d_pixels is NULL");
  if (capacity > 0 && ((uintptr_t)d_pixels & 7u)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "select_pixels: d_pixels must be 8-byte aligned");
  Texture* c = find_texture(ctx, count);
  if (!c) return fail(ctx, URT_ERR_INVALID_HANDLE, "select_pixels: unknown count texture handle");
  if (int rc = check_select_size(ctx, "select_pixels", c)) return rc;
  URT_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n_texels = (size_t)c->w * (size_t)c->h;
  if (int rc = select_scratch(ctx, "select_pixels: scratch allocation", n_texels)) return rc;
  { int rc = flush_pending(ctx); if (rc) return rc; }
  URT_HIP(ctx, launch_select_count(c->dev, n_texels, below, ctx->rs_counts.get(), touch(ctx)));   // the device pointer after the flush (a Result texture may be renamed)
  URT_HIP(ctx, launch_select_write(c->dev, c->w, n_texels, below, ctx->rs_counts.get(), (int2*)d_pixels, capacity, touch(ctx)));
  int total = 0;
  if (int rc = select_total(ctx, n_texels, &total)) return rc;
  *out_n = total;
  return URT_OK;
  URT_GUARD_END(ctx)
}

// urt_blend_samples writes dst and count: checked first, then the deferred frames are submitted and k_blend_samples is enqueued.
int urt_blend_samples(urt_context* ctx, const void* d_pixels, const void* d_samples, int n, float weight, urt_handle dst, urt_handle count,
                      float max_history) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  if (n < 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "blend_samples: negative sample count");
  if (n > 0 && (!d_pixels || !d_samples)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "blend_samples: d_pixels / d_samples is NULL");
  if (n > 0 && (((uintptr_t)d_pixels & 7u) || ((uintptr_t)d_samples & 15u)))
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "blend_samples: d_pixels must be 8-byte aligned, d_samples 16-byte aligned");
  if (int rc = check_blend_numbers(ctx, "blend_samples", weight, max_history)) return rc;
  Texture* t[2];
  if (int rc = resolve_blend_targets(ctx, "blend_samples", dst, count, t)) return rc;
  if (n == 0) return URT_OK;
  URT_HIP(ctx, hipSetDevice(ctx->device));
  { int rc = flush_pending(ctx); if (rc) return rc; }
  t[0]->other_writes = true;
  t[1]->other_writes = true;
  URT_HIP(ctx, launch_blend_samples((const int2*)d_pixels, (const float4*)d_samples, n, weight, t[0]->dev, t[1]->dev, t[0]->w, t[0]->h,
                                    max_history, touch(ctx)));
  return URT_OK;
  URT_GUARD_END(ctx)
}

// The three steps in one call, for hosts without device pointers: count + scan, ONE synchronisation for the selected count n, then the
// scratch for n pixels and n samples, the write phase, the radiance query (pixels mode, device form) and the blend, all only enqueued.
// Everything the three separate calls would refuse is refused before anything is enqueued.
int urt_resample_below(urt_context* ctx, urt_handle dst, urt_handle count, float below, int samples, int bounces, float weight,
                       float max_history, int* out_n) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  if (std::isnan(below)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "resample_below: below is NaN");
  if (samples < 1 || samples > 4096) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "resample_below: samples must be 1..4096");
  if (bounces < 0 || bounces > 64) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "resample_below: bounces must be 0..64");
  if (int rc = check_blend_numbers(ctx, "resample_below", weight, max_history)) return rc;
  Texture* t[2];
  if (int rc = resolve_blend_targets(ctx, "resample_below", dst, count, t)) return rc;
  if (int rc = check_select_size(ctx, "resample_below", t[1])) return rc;
  const Texture* res = find_texture(ctx, ctx->t_result);
  if (!res) return fail(ctx, URT_ERR_UNBOUND, "resample_below: no texture bound to \"Result\"");
  if (!ctx->c2w_set || !ctx->invp_set)
    return fail(ctx, URT_ERR_UNBOUND, "resample_below: _CameraToWorld / _CameraInverseProjection not set");
  if (res->w != t[0]->w || res->h != t[0]->h)
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "resample_below: dst and count must have the size of the texture bound as Result");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  const int width = t[1]->w, height = t[1]->h;
  const size_t n_texels = (size_t)width * (size_t)height;
  if (int rc = select_scratch(ctx, "resample_below: scratch allocation", n_texels)) return rc;
  { int rc = flush_pending(ctx); if (rc) return rc; }
  URT_HIP(ctx, launch_select_count(t[1]->dev, n_texels, below, ctx->rs_counts.get(), touch(ctx)));
  int n = 0;
  if (int rc = select_total(ctx, n_texels, &n)) return rc;
  if (out_n) *out_n = n;
  if (n == 0) return URT_OK;
  if (int rc = reserve(ctx, ctx->rs_pixels, (size_t)n, "resample_below: scratch allocation", ctx->stream)) return rc;
  if (int rc = reserve(ctx, ctx->rs_samples, (size_t)n, "resample_below: scratch allocation", ctx->stream)) return rc;
  URT_HIP(ctx, launch_select_write(t[1]->dev, width, n_texels, below, ctx->rs_counts.get(), (int2*)ctx->rs_pixels.get(), n, touch(ctx)));
  DevScene S; FrameUniforms C; RadianceBatch B;
  if (int rc = radiance_prepare(ctx, ctx->rs_pixels.get(), n, samples, bounces, ctx->rs_samples.get(), URT_RADIANCE_PIXELS, false, &S, &C, &B)) return rc;
  B.in = ctx->rs_pixels.get(); B.out = ctx->rs_samples.get();
  URT_HIP(ctx, launch_radiance(S, lane_stack_size(ctx), C, B, touch(ctx)));
  Texture* d = find_texture(ctx, dst);
  Texture* c = find_texture(ctx, count);
  if (!d || !c) return fail(ctx, URT_ERR_INVALID_HANDLE, "resample_below: a texture was released during the call");
  d->other_writes = true;
  c->other_writes = true;
  URT_HIP(ctx, launch_blend_samples((const int2*)ctx->rs_pixels.get(), ctx->rs_samples.get(), n, weight, d->dev, c->dev, width, height, max_history, touch(ctx)));
  return URT_OK;
  URT_GUARD_END(ctx)
}

}  // extern "C"
