// context.cpp — implementation of the C ABI in include/urt.h: the context and the objects it hands out (the other files: context_impl.h).
//
// Stands in for the UnityEngine GPU objects RayTraceMaster.cs drives:
//   ComputeBuffer   -> Buffer   (host copy kept; the device form is DERIVED at the next dispatch; an optional device mirror takes
//                                device-side writes: urt_buffer_set_data_device and urt_buffer_copy here, the calls of geometry_ops.cpp)
//   RenderTexture   -> Texture  (RGBA32F device image)
//   ComputeShader   -> the uniform/binding table in urt_context + dispatch of the HIP kernels
//   Graphics.Blit   -> urt_blit / urt_blit_add
// There is deliberately no CPU path: without a HIP device context creation fails.
#include "experiments.h"
#include "context_impl.h"
#include "tile_entry.h"

#include <climits>
#include <memory>

#include "index_span.h"
#include "present.h"
#include "reproject.h"

using namespace urtd;

namespace {

const char* const kBindNames[B_COUNT] = {"_MeshObjects", "_Vertices", "_Indices", "_Normals", "_Spheres", "_MeshBVH", "_SphereBVH"};
const int kBindStride[B_COUNT] = {URT_STRIDE_MESHOBJECT, URT_STRIDE_VEC3, URT_STRIDE_INDEX, URT_STRIDE_VEC3,
                                  URT_STRIDE_SPHERE, URT_STRIDE_BVHNODE, URT_STRIDE_BVHNODE};

std::string g_create_error;   // urt_last_error(NULL)

// process-wide cache for urt_debug_build_blas / urt_debug_get_blas
BlasResult g_debug_blas;

}  // namespace

namespace urtd {

int fail(urt_context* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg; else g_create_error = msg;
  return code;
}

// After the stream has been waited for: did a wave of the work just completed leave through a cap?
int check_watchdog(urt_context* ctx) {
  if (!ctx->h_trip_flag) return URT_OK;
  unsigned int n = __atomic_exchange_n(ctx->h_trip_flag.get(), 0u, __ATOMIC_ACQ_REL);
  if (n == 0) return URT_OK;
  return fail(ctx, URT_ERR_WATCHDOG, std::to_string(n) + " wave(s) of a trace launch hit the kernel's iteration cap and left pixels unwritten "
                                     "(urt_counters.watchdog_trips): the images written since the last successful synchronisation are incomplete");
}

// D2H of elements first .. last of the mirror into `host`: synchronises (the stream carries the kernels that wrote them) and is counted.
int download_elements(urt_context* ctx, Buffer& b, int first, int last) {
  const size_t at = (size_t)first * (size_t)b.stride, bytes = (size_t)(last - first + 1) * (size_t)b.stride;
  URT_HIP(ctx, hipSetDevice(ctx->device));
  URT_HIP(ctx, hipMemcpyAsync(b.host.data() + at, b.mirror.get() + at, bytes, hipMemcpyDeviceToHost, touch(ctx)));
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  b.downloads++;
  return URT_OK;
}

// `host` made current: the stale range comes down (nothing to do without one)
int buffer_sync_host(urt_context* ctx, Buffer& b) {
  if (!b.stale() || !b.mirror) return URT_OK;
  if (int rc = download_elements(ctx, b, b.stale_first, b.stale_last)) return rc;
  b.stale_first = 0; b.stale_last = -1;
  return URT_OK;
}
int sync_bound_hosts(urt_context* ctx, unsigned int slots) {
  for (int s = 0; s < B_COUNT; s++) {
    Buffer* b = (slots >> s) & 1u ? find_buffer(ctx, ctx->bound[s]) : nullptr;
    if (b) if (int rc = buffer_sync_host(ctx, *b)) return rc;
  }
  return URT_OK;
}

// The mirror, made and filled from `host` at the first need: a synchronous copy, before anything on the stream can use the new memory.
int buffer_mirror(urt_context* ctx, Buffer& b) {
  if (b.mirror) return URT_OK;
  const size_t bytes = (size_t)b.count * (size_t)b.stride;
  URT_HIP(ctx, hipSetDevice(ctx->device));
  URT_HIP(ctx, b.mirror.alloc(bytes));
  hipError_t e = hipMemcpy(b.mirror.get(), b.host.data(), bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) { b.mirror.reset(); return fail(ctx, URT_ERR_HIP, std::string("buffer mirror upload: ") + hipGetErrorString(e)); }
  return URT_OK;
}

// strips first_row, first_row + row_stride, ... of 8-row groups that lie in the first group_rows
int strip_count(int group_rows, int first_row, int row_stride) {
  return first_row < group_rows ? (group_rows - first_row + row_stride - 1) / row_stride : 0;
}

// Elements first .. last have changed: they join the dirty range, and every slot the buffer is bound to asks for a preparation.
static void mark_changed(urt_context* ctx, urt_handle buffer, Buffer& b, int first, int last) {
  b.mark_dirty(first, last);
  for (int s = 0; s < B_COUNT; s++) if (ctx->bound[s] == buffer) { ctx->scene_dirty = true; ctx->dirty_slots |= 1u << s; }
}

// A device-side writer has filled elements first .. first + count - 1 of the mirror (count > 0): `host` is behind there, and every element
// counts as changed.
void mark_device_written(urt_context* ctx, urt_handle buffer, Buffer& b, int first, int count) {
  const bool fresh = !b.has_data;                            // set for the first time: new as a whole, as with SetData
  b.has_data = true;
  b.mark_stale(first, first + count - 1);
  mark_changed(ctx, buffer, b, fresh ? 0 : first, fresh ? b.count - 1 : first + count - 1);
}

int check_element_range(urt_context* ctx, const char* who, const Buffer& b, int first, int count) {
  if (first < 0 || count < 0 || (long long)first + (long long)count > (long long)b.count)
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string(who) + ": the element range lies outside the buffer");
  return URT_OK;
}

}  // namespace urtd

extern "C" {

int urt_abi_version(void) { return URT_ABI_SIGN * 4; }   // negative: an A/B / probe / diagnostic build (csrc/experiments.h), refused by loaders that did not opt in

int urt_device_count(int* out_count) {
  if (!out_count) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "out_count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *out_count = 0; return fail(nullptr, URT_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
  *out_count = n;
  return URT_OK;
}

int urt_context_create(int device, urt_context** out_ctx) {
  if (!out_ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "out_ctx is NULL");
  *out_ctx = nullptr;
  URT_GUARD_BEGIN
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(nullptr, URT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= n) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "device ordinal out of range");
  URT_HIP(nullptr, hipSetDevice(device));
  std::unique_ptr<urt_context> ctx(new urt_context());
  ctx->device = device;
  e = ctx->own_stream.create(hipStreamNonBlocking);
  if (e != hipSuccess) return fail(nullptr, URT_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  ctx->stream = ctx->own_stream.get();
  e = ctx->d_counters.alloc(kCounterShards);
  if (e == hipSuccess) e = hipMemset(ctx->d_counters.get(), 0, sizeof(DevCounters) * kCounterShards);
  for (auto* next : {&ctx->d_next, &ctx->d_next2}) {       // d_next2: the launch on the second trace stream (same layout)
    if (e == hipSuccess) e = next->alloc(urt_context::kWorkCounterBytes / sizeof(unsigned int));
    if (e == hipSuccess) e = hipMemset(next->get(), 0, urt_context::kWorkCounterBytes);
  }
  if (e == hipSuccess) e = ctx->h_trip_flag.alloc(1, 64, hipHostMallocMapped | hipHostMallocCoherent);   // the watchdog word the kernels raise (system-scope atomic)
  if (e == hipSuccess) { *ctx->h_trip_flag.get() = 0; e = hipHostGetDevicePointer((void**)&ctx->d_trip_flag, ctx->h_trip_flag.get(), 0); }
  if (e == hipSuccess) { int n = 0; if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) ctx->n_cus = n; }
  if (e != hipSuccess) return fail(nullptr, URT_ERR_HIP, std::string("counter allocation: ") + hipGetErrorString(e));
  *out_ctx = ctx.release();
  return URT_OK;
  URT_GUARD_END(nullptr)
}

// What destructors cannot order is done by hand: the deferred work is submitted and waited for on every stream that carries some
// (main, copy, trace) before any holder gives its resource back.
int urt_context_destroy(urt_context* ctx) {
  if (!ctx) return URT_OK;
  (void)hipSetDevice(ctx->device);
  (void)flush_pending(ctx);
  (void)hipStreamSynchronize(touch(ctx));
  resolve_timing(ctx);
  for (auto& r : ctx->rslot) if (r.done) (void)hipEventSynchronize(r.done.get());
  for (auto& q : ctx->trace_q) if (q) (void)hipStreamSynchronize(q.get());
  free_scene(ctx);
  delete ctx;
  return URT_OK;
}

const char* urt_last_error(urt_context* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int urt_context_set_stream(urt_context* ctx, void* hip_stream) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  { int rc = flush_pending(ctx); if (rc) return rc; }
  hipStream_t to = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream.get();
  if (to == ctx->stream) return URT_OK;
  // no host synchronisation: everything issued so far on the old stream is ordered before whatever is issued on the new
  // one by an event (a caller that ping-pongs between a render and a communication stream must not stall on either)
  if (!ctx->ev_switch) URT_HIP(ctx, ctx->ev_switch.create(hipEventDisableTiming));
  URT_HIP(ctx, hipEventRecord(ctx->ev_switch.get(), touch(ctx)));
  URT_HIP(ctx, hipStreamWaitEvent(to, ctx->ev_switch.get(), 0));
  ctx->stream = to;
  return URT_OK;
}

int urt_flush(urt_context* ctx) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  return flush_pending(ctx);
  URT_GUARD_END(ctx)
}

int urt_synchronize(urt_context* ctx) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  { int rc = flush_pending(ctx); if (rc) return rc; }
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  return check_watchdog(ctx);
}

/* ---- ComputeBuffer ---- */
int urt_buffer_create(urt_context* ctx, int count, int stride, urt_handle* out_buffer) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!out_buffer) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "out_buffer is NULL");
  // Unity: "ComputeBuffer count/stride must be greater than 0" and stride a multiple of 4
  if (count <= 0 || stride <= 0 || (stride & 3)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "ComputeBuffer: count and stride must be > 0 and stride a multiple of 4");
  URT_GUARD_BEGIN
  Buffer b; b.count = count; b.stride = stride;
  b.host.assign((size_t)count * (size_t)stride, 0);
  urt_handle h = ctx->next_id++;
  ctx->buffers.emplace(h, std::move(b));
  *out_buffer = h;
  return URT_OK;
  URT_GUARD_END(ctx)
}

// The first and the last byte at which two ranges differ (false: they are equal): two passes of memcmp over blocks, then over bytes,
// which costs what the one memcmp of equal data would.
static bool differing_bytes(const uint8_t* a, const uint8_t* b, size_t n, size_t* first, size_t* last) {
  constexpr size_t kBlock = 4096;
  size_t i = 0;
  while (i < n) { size_t len = std::min(kBlock, n - i); if (std::memcmp(a + i, b + i, len) != 0) break; i += len; }
  if (i >= n) return false;
  while (a[i] == b[i]) i++;
  size_t j = n;
  while (j > i + 1) { size_t len = std::min(kBlock, j - (i + 1)); if (std::memcmp(a + j - len, b + j - len, len) != 0) break; j -= len; }
  while (j > i + 1 && a[j - 1] == b[j - 1]) j--;
  *first = i; *last = j - 1;
  return true;
}

// ---- device mirrors (context_impl.h Buffer::mirror; buffer_mirror above) ---------------------------------------------------------------
// Host elements first .. last -> mirror, on the stream, through a pinned image: the caller may change `host` as soon as this returns, and
// nothing but the slot's own previous copy is waited for.
static int push_elements(urt_context* ctx, Buffer& b, int first, int last) {
  const size_t at = (size_t)first * (size_t)b.stride, bytes = (size_t)(last - first + 1) * (size_t)b.stride;
  URT_HIP(ctx, hipSetDevice(ctx->device));
  urt_context::UpSlot& u = ctx->up_slot[ctx->up_next++ % urt_context::kUpSlots];
  if (!u.done) URT_HIP(ctx, u.done.create(hipEventDisableTiming));
  if (u.used) URT_HIP(ctx, hipEventSynchronize(u.done.get()));
  if (u.host.cap() < bytes) { u.used = false; URT_HIP(ctx, u.host.alloc(bytes)); }
  std::memcpy(u.host.get(), b.host.data() + at, bytes);
  URT_HIP(ctx, hipMemcpyAsync(b.mirror.get() + at, u.host.get(), bytes, hipMemcpyHostToDevice, touch(ctx)));
  URT_HIP(ctx, hipEventRecord(u.done.get(), ctx->stream));
  u.used = true;
  return URT_OK;
}

// SetData of elements first .. first + count - 1 (arguments checked by the callers): data equal to what the buffer holds changes nothing and
// dirties nothing (the reference re-uploads EVERY list whenever anything changed, RM:738-745; a compare costs what the copy would);
// else the elements between the first and the last differing byte join the buffer's dirty range.  Elements inside the stale range differ
// by definition (the compare does not download): they leave the stale range, and when that would split it in two the part behind the
// written elements is downloaded first.  What changed is pushed into the mirror, if there is one.
static int set_data_elements(urt_context* ctx, urt_handle buffer, Buffer& b, int first, const void* data, int count) {
  const size_t bytes = (size_t)count * (size_t)b.stride, at = (size_t)first * (size_t)b.stride;
  const int last = first + count - 1;
  int d0 = 0, d1 = b.count - 1;                              // a buffer that is set for the first time is new as a whole
  int p0 = first, p1 = last;                                 // what the mirror lacks
  const int s0 = std::max(first, b.stale_first), s1 = std::min(last, b.stale_last);
  const bool meets_stale = count > 0 && b.stale() && s0 <= s1;
  if (b.has_data) {
    size_t f = 0, l = 0;
    const bool differs = bytes > 0 && differing_bytes(b.host.data() + at, (const uint8_t*)data, bytes, &f, &l);
    if (!differs && !meets_stale) return URT_OK;
    if (differs) { d0 = first + (int)(f / (size_t)b.stride); d1 = first + (int)(l / (size_t)b.stride); }
    if (meets_stale) { d0 = differs ? std::min(d0, s0) : s0; d1 = differs ? std::max(d1, s1) : s1; }
    p0 = d0; p1 = d1;
  }
  if (meets_stale) {
    if (b.stale_first < first && last < b.stale_last) {
      if (int rc = download_elements(ctx, b, last + 1, b.stale_last)) return rc;
      b.stale_last = first - 1;
    } else if (b.stale_first >= first && b.stale_last <= last) { b.stale_first = 0; b.stale_last = -1; }
    else if (b.stale_first < first) b.stale_last = first - 1;
    else b.stale_first = last + 1;
  }
  if (bytes > 0) std::memcpy(b.host.data() + at, data, bytes);
  b.has_data = true;
  if (b.mirror && bytes > 0) if (int rc = push_elements(ctx, b, p0, p1)) return rc;
  mark_changed(ctx, buffer, b, d0, d1);
  return URT_OK;
}

int urt_buffer_set_data(urt_context* ctx, urt_handle buffer, const void* data, int count) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  auto it = ctx->buffers.find(buffer);
  if (it == ctx->buffers.end()) return fail(ctx, URT_ERR_INVALID_HANDLE, "SetData: unknown buffer handle");
  Buffer& b = it->second;
  if (count < 0 || count > b.count) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "SetData: more elements than the buffer holds");
  if (count > 0 && !data) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "SetData: data is NULL");
  return set_data_elements(ctx, buffer, b, 0, data, count);
}

int urt_buffer_set_data_range(urt_context* ctx, urt_handle buffer, int first, const void* data, int count) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  auto it = ctx->buffers.find(buffer);
  if (it == ctx->buffers.end()) return fail(ctx, URT_ERR_INVALID_HANDLE, "SetData: unknown buffer handle");
  Buffer& b = it->second;
  if (first < 0 || count < 0 || (long long)first + (long long)count > (long long)b.count)
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "SetData: the element range lies outside the buffer");
  if (count > 0 && !data) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "SetData: data is NULL");
  if (count == 0) return URT_OK;
  return set_data_elements(ctx, buffer, b, first, data, count);
}

int urt_buffer_set_data_device(urt_context* ctx, urt_handle buffer, int first, const void* d_data, int count) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  Buffer* b = find_buffer(ctx, buffer);
  if (!b) return fail(ctx, URT_ERR_INVALID_HANDLE, "SetDataDevice: unknown buffer handle");
  if (int rc = check_element_range(ctx, "SetDataDevice", *b, first, count)) return rc;
  if (count > 0 && (!d_data || ((uintptr_t)d_data & 3u))) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "SetDataDevice: d_data is NULL or not 4-byte aligned");
  if (count == 0) return URT_OK;
  URT_GUARD_BEGIN
  if (int rc = buffer_mirror(ctx, *b)) return rc;
  const size_t at = (size_t)first * (size_t)b->stride, bytes = (size_t)count * (size_t)b->stride;
  URT_HIP(ctx, hipMemcpyAsync(b->mirror.get() + at, d_data, bytes, hipMemcpyDeviceToDevice, touch(ctx)));
  mark_device_written(ctx, buffer, *b, first, count);
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_buffer_copy(urt_context* ctx, urt_handle src, int src_first, urt_handle dst, int dst_first, int count) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  Buffer* s = find_buffer(ctx, src);
  Buffer* d = find_buffer(ctx, dst);
  if (!s || !d) return fail(ctx, URT_ERR_INVALID_HANDLE, std::string("buffer_copy: ") + (!s ? "src" : "dst") + " is 0 or an unknown buffer handle");
  if (src == dst) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "buffer_copy: src and dst are one buffer");
  if (s->stride != d->stride) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "buffer_copy: the strides of src and dst differ");
  if (int rc = check_element_range(ctx, "buffer_copy (src)", *s, src_first, count)) return rc;
  if (int rc = check_element_range(ctx, "buffer_copy (dst)", *d, dst_first, count)) return rc;
  if (count == 0) return URT_OK;
  URT_GUARD_BEGIN
  if (int rc = buffer_mirror(ctx, *s)) return rc;
  if (int rc = buffer_mirror(ctx, *d)) return rc;
  const size_t bytes = (size_t)count * (size_t)s->stride;
  URT_HIP(ctx, hipMemcpyAsync(d->mirror.get() + (size_t)dst_first * (size_t)d->stride, s->mirror.get() + (size_t)src_first * (size_t)s->stride, bytes,
                              hipMemcpyDeviceToDevice, touch(ctx)));
  mark_device_written(ctx, dst, *d, dst_first, count);
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_buffer_get_data_range(urt_context* ctx, urt_handle buffer, int first, void* out, int count) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  Buffer* b = find_buffer(ctx, buffer);
  if (!b) return fail(ctx, URT_ERR_INVALID_HANDLE, "GetData: unknown buffer handle");
  if (int rc = check_element_range(ctx, "GetData", *b, first, count)) return rc;
  if (count > 0 && !out) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "GetData: out is NULL");
  if (count == 0) return URT_OK;
  if (b->stale() && first <= b->stale_last && first + count - 1 >= b->stale_first)
    if (int rc = buffer_sync_host(ctx, *b)) return rc;
  std::memcpy(out, b->host.data() + (size_t)first * (size_t)b->stride, (size_t)count * (size_t)b->stride);
  return URT_OK;
}

int urt_debug_buffer_state(urt_context* ctx, urt_handle buffer, uint64_t out4[4]) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  const Buffer* b = find_buffer(ctx, buffer);
  if (!b) return fail(ctx, URT_ERR_INVALID_HANDLE, "buffer_state: unknown buffer handle");
  if (!out4) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "buffer_state: out4 is NULL");
  out4[0] = b->stale() ? (uint64_t)b->stale_first : 1; out4[1] = b->stale() ? (uint64_t)b->stale_last : 0;
  out4[2] = b->mirror ? (uint64_t)b->count * (uint64_t)b->stride : 0;
  out4[3] = b->downloads;
  return URT_OK;
}

int urt_buffer_get_info(urt_context* ctx, urt_handle buffer, int* out_count, int* out_stride) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  auto it = ctx->buffers.find(buffer);
  if (it == ctx->buffers.end()) return fail(ctx, URT_ERR_INVALID_HANDLE, "unknown buffer handle");
  if (out_count) *out_count = it->second.count;
  if (out_stride) *out_stride = it->second.stride;
  return URT_OK;
}

int urt_buffer_release(urt_context* ctx, urt_handle buffer) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  auto it = ctx->buffers.find(buffer);
  if (it == ctx->buffers.end()) return fail(ctx, URT_ERR_INVALID_HANDLE, "Release: unknown buffer handle");
  for (int s = 0; s < B_COUNT; s++) if (ctx->bound[s] == buffer) { ctx->bound[s] = 0; ctx->scene_dirty = true; ctx->dirty_full = true; }
  if (it->second.mirror) {                                   // kernels and copies queued on the stream may still use the mirror
    URT_HIP(ctx, hipSetDevice(ctx->device));
    URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  }
  ctx->buffers.erase(it);
  return URT_OK;
}

/* ---- textures ---- */
static int texture_create_impl(urt_context* ctx, int width, int height, void* ext, urt_handle* out_texture) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!out_texture) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "out_texture is NULL");
  if (width <= 0 || height <= 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "texture size must be positive");
  URT_GUARD_BEGIN
  URT_HIP(ctx, hipSetDevice(ctx->device));
  Texture t; t.w = width; t.h = height;
  size_t bytes = (size_t)width * (size_t)height * sizeof(float4);
  if (ext) { t.dev = (float4*)ext; t.external = true; t.other_writes = true; /* caller memory: contents unknown */ }
  else {
    URT_HIP(ctx, t.storage.alloc((size_t)width * (size_t)height));
    t.dev = t.storage.get();
    hipError_t e = hipMemsetAsync(t.dev, 0, bytes, touch(ctx));
    if (e != hipSuccess) return fail(ctx, URT_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
  }
  t.own = t.dev;
  urt_handle h = ctx->next_id++;
  ctx->textures.emplace(h, std::move(t));
  *out_texture = h;
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_texture_create(urt_context* ctx, int width, int height, urt_handle* out_texture) {
  return texture_create_impl(ctx, width, height, nullptr, out_texture);
}

int urt_texture_create_external(urt_context* ctx, int width, int height, void* device_ptr, urt_handle* out_texture) {
  if (ctx && !device_ptr) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "device_ptr is NULL");
  return texture_create_impl(ctx, width, height, device_ptr, out_texture);
}

int urt_texture_set_pixels(urt_context* ctx, urt_handle texture, const float* rgba) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  Texture* t = find_texture(ctx, texture);
  if (!t) return fail(ctx, URT_ERR_INVALID_HANDLE, "unknown texture handle");
  if (!rgba) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "rgba is NULL");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  { int rc = flush_pending(ctx); if (rc) return rc; }
  t->other_writes = true;
  URT_HIP(ctx, hipMemcpyAsync(t->dev, rgba, (size_t)t->w * t->h * sizeof(float4), hipMemcpyHostToDevice, touch(ctx)));
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  return URT_OK;
}

int urt_texture_get_pixels(urt_context* ctx, urt_handle texture, float* rgba) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  Texture* t = find_texture(ctx, texture);
  if (!t) return fail(ctx, URT_ERR_INVALID_HANDLE, "unknown texture handle");
  if (!rgba) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "rgba is NULL");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  { int rc = flush_pending(ctx); if (rc) return rc; }
  URT_HIP(ctx, hipMemcpyAsync(rgba, t->dev, (size_t)t->w * t->h * sizeof(float4), hipMemcpyDeviceToHost, touch(ctx)));
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  return check_watchdog(ctx);                           // pixels of a launch that hit a cap are not handed out as good
}

// Pipelined readback.  begin: the image as it is at this point of the program order is snapshot on the render stream (a device-to-device
// copy: 33 MB at 1080p, ~20 us) and travels to a pinned host image on a stream of its own, so the frames dispatched AFTER the call render
// while it is on the PCIe bus; end: waits for that one copy and hands the pinned image out.
int urt_texture_read_begin(urt_context* ctx, urt_handle texture, uint64_t* out_ticket) { return urt_texture_read_begin_format(ctx, texture, URT_FORMAT_RGBA32F, out_ticket); }

// ... in the format of the host's `destination` (csrc/present.hip): the snapshot on the render stream IS the conversion kernel (16 B read,
// 4 or 8 B written per pixel), and only the converted image crosses the bus.
int urt_texture_read_begin_format(urt_context* ctx, urt_handle texture, int format, uint64_t* out_ticket) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!out_ticket) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "out_ticket is NULL");
  const size_t bpp = urtd::format_pixel_bytes(format);
  if (!bpp) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "urt_texture_read_begin_format: format must be URT_FORMAT_RGBA32F, _RGBA8_SRGB or _RGBA16F");
  Texture* t = find_texture(ctx, texture);
  if (!t) return fail(ctx, URT_ERR_INVALID_HANDLE, "unknown texture handle");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  { int rc = flush_pending(ctx); if (rc) return rc; }
  t = find_texture(ctx, texture);
  if (!ctx->copy_stream) URT_HIP(ctx, ctx->copy_stream.create(hipStreamNonBlocking));
  urt_context::ReadSlot& r = ctx->rslot[ctx->read_next % urt_context::kReadSlots];
  if (r.busy) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "urt_texture_read_begin: three readbacks are in flight — end the oldest first");
  const size_t px = (size_t)t->w * (size_t)t->h;
  if (r.dev.cap() < px || r.host.cap() < px) {               // the pair grows together, after the slot's last copy
    if (r.done) URT_HIP(ctx, hipEventSynchronize(r.done.get()));
    URT_HIP(ctx, r.dev.alloc(px));
    URT_HIP(ctx, r.host.alloc(px));
  }
  if (!r.snap) { URT_HIP(ctx, r.snap.create(hipEventDisableTiming)); URT_HIP(ctx, r.done.create(hipEventDisableTiming)); }
  if (format == urtd::kFormatRGBA32F) {
    URT_HIP(ctx, hipMemcpyAsync(r.dev.get(), t->dev, px * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
  } else {
    if (format == urtd::kFormatRGBA8sRGB && !ctx->srgb_first) {
      float first[urtd::kSrgbCodes];
      (void)urt_host_srgb8_first_floats(first);
      URT_HIP(ctx, ctx->srgb_first.alloc(urtd::kSrgbCodes));
      URT_HIP(ctx, hipMemcpy(ctx->srgb_first.get(), first, sizeof(first), hipMemcpyHostToDevice));
    }
    URT_HIP(ctx, urtd::launch_encode(t->dev, r.dev.get(), px, format, ctx->srgb_first.get(), ctx->stream));
  }
  r.format = format;
  r.bytes = px * bpp;
  URT_HIP(ctx, hipEventRecord(r.snap.get(), ctx->stream));
  URT_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream.get(), r.snap.get(), 0));
  URT_HIP(ctx, hipMemcpyAsync(r.host.get(), r.dev.get(), r.bytes, hipMemcpyDeviceToHost, ctx->copy_stream.get()));
  URT_HIP(ctx, hipEventRecord(r.done.get(), ctx->copy_stream.get()));
  r.busy = true;
  r.ticket = ++ctx->read_next;                               // tickets start at 1; slot = (ticket - 1) % kReadSlots
  *out_ticket = r.ticket;
  return URT_OK;
}

int urt_texture_read_end(urt_context* ctx, uint64_t ticket, const float** out_rgba) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!out_rgba || ticket == 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "bad ticket / out_rgba is NULL");
  urt_context::ReadSlot& r = ctx->rslot[(ticket - 1) % urt_context::kReadSlots];
  if (r.busy && r.ticket == ticket && r.format != urtd::kFormatRGBA32F)
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "urt_texture_read_end: this ticket holds a converted image — end it with urt_texture_read_end_format");
  const void* p = nullptr;
  int rc = urt_texture_read_end_format(ctx, ticket, &p, nullptr);
  if (rc == URT_OK || rc == URT_ERR_WATCHDOG) *out_rgba = (const float*)p;
  return rc;
}

int urt_texture_read_end_format(urt_context* ctx, uint64_t ticket, const void** out_pixels, size_t* out_bytes) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!out_pixels || ticket == 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "bad ticket / out_pixels is NULL");
  urt_context::ReadSlot& r = ctx->rslot[(ticket - 1) % urt_context::kReadSlots];
  if (!r.busy || r.ticket != ticket) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "urt_texture_read_end: this ticket is not in flight");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  URT_HIP(ctx, hipEventSynchronize(r.done.get()));
  r.busy = false;
  *out_pixels = r.host.get();                                      // valid until the third urt_texture_read_begin after this one
  if (out_bytes) *out_bytes = r.bytes;
  return check_watchdog(ctx);
}

int urt_texture_get_info(urt_context* ctx, urt_handle texture, int* out_width, int* out_height, void** out_device_ptr) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  Texture* t = find_texture(ctx, texture);
  if (!t) return fail(ctx, URT_ERR_INVALID_HANDLE, "unknown texture handle");
  if (out_width) *out_width = t->w;
  if (out_height) *out_height = t->h;
  if (out_device_ptr) {
    // the caller is going to touch the memory itself: submit what is deferred, give the image back its own (stable)
    // storage and never rename it again
    URT_HIP(ctx, hipSetDevice(ctx->device));
    int rc = flush_pending(ctx); if (rc) return rc;
    rc = detach_from_slab(ctx, *t); if (rc) return rc;
    t->ptr_exposed = true;
    *out_device_ptr = t->dev;
  }
  return URT_OK;
}

int urt_texture_release(urt_context* ctx, urt_handle texture) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  auto it = ctx->textures.find(texture);
  if (it == ctx->textures.end()) return fail(ctx, URT_ERR_INVALID_HANDLE, "Release: unknown texture handle");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  { int rc = flush_pending(ctx); if (rc) return rc; }
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  ctx->slab_oom_stride = 0;                                // device memory came back: the next batch may try the Result slots again
  if (ctx->slab_tex == texture) ctx->slab_tex = 0;
  if (ctx->t_sky == texture) ctx->t_sky = 0;
  if (ctx->t_result == texture) ctx->t_result = 0;
  ctx->textures.erase(it);
  return URT_OK;
}

/* ---- shader uniforms and bindings ---- */
int urt_shader_set_buffer(urt_context* ctx, int kernel, const char* name, urt_handle buffer) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (kernel != 0 || !name) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "SetBuffer: kernel must be 0 and name non-NULL");
  for (int s = 0; s < B_COUNT; s++) {
    if (std::strcmp(name, kBindNames[s]) != 0) continue;
    if (buffer) {
      auto it = ctx->buffers.find(buffer);
      if (it == ctx->buffers.end()) return fail(ctx, URT_ERR_INVALID_HANDLE, "SetBuffer: unknown buffer handle");
      if (it->second.stride != kBindStride[s])
        return fail(ctx, URT_ERR_LAYOUT, std::string("SetBuffer(") + name + "): stride " + std::to_string(it->second.stride) +
                                             " != " + std::to_string(kBindStride[s]) + " (RM:738-745)");
    }
    if (ctx->bound[s] != buffer) { ctx->bound[s] = buffer; ctx->scene_dirty = true; ctx->dirty_full = true; }   // re-binding the same buffer every frame (RM:787-794) is free
    return URT_OK;
  }
  return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string("SetBuffer: kernel CSMain has no buffer named ") + name);
}

int urt_shader_set_texture(urt_context* ctx, int kernel, const char* name, urt_handle texture) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (kernel != 0 || !name) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "SetTexture: kernel must be 0 and name non-NULL");
  if (texture && !find_texture(ctx, texture)) return fail(ctx, URT_ERR_INVALID_HANDLE, "SetTexture: unknown texture handle");
  if (std::strcmp(name, "_SkyboxTexture") == 0) { ctx->t_sky = texture; return URT_OK; }
  if (std::strcmp(name, "Result") == 0) { ctx->t_result = texture; return URT_OK; }
  return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string("SetTexture: kernel CSMain has no texture named ") + name);
}

int urt_shader_set_matrix(urt_context* ctx, const char* name, const float* m16) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!name || !m16) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "SetMatrix: NULL argument");
  if (std::strcmp(name, "_CameraToWorld") == 0) { std::memcpy(ctx->c2w, m16, sizeof ctx->c2w); ctx->c2w_set = true; }
  else if (std::strcmp(name, "_CameraInverseProjection") == 0) { std::memcpy(ctx->invp, m16, sizeof ctx->invp); ctx->invp_set = true; }
  return URT_OK;   // undeclared names are ignored, as Unity does
}

int urt_shader_set_vector(urt_context* ctx, const char* name, const float* v4) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!name || !v4) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "SetVector: NULL argument");
  if (std::strcmp(name, "_PixelOffset") == 0) { ctx->pixel_off[0] = v4[0]; ctx->pixel_off[1] = v4[1]; }
  return URT_OK;
}

int urt_shader_set_float(urt_context* ctx, const char* name, float value) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!name) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "SetFloat: NULL name");
  if (std::strcmp(name, "_Seed") == 0) ctx->seed = value;
  return URT_OK;
}

int urt_shader_set_int(urt_context* ctx, const char* name, int value) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!name) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "SetInt: NULL name");
  if (std::strcmp(name, "_numBounces") == 0) ctx->num_bounces = value;
  else if (std::strcmp(name, "_numRays") == 0) ctx->num_rays = value;
  // "_MeshBVH_len" / "_SphereBVH_len": static const in the shader (RS:73-74) — accepted, no effect
  return URT_OK;
}

int urt_shader_dispatch(urt_context* ctx, int kernel, int groups_x, int groups_y, int groups_z) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  return do_dispatch(ctx, kernel, groups_x, groups_y, groups_z, 0, 1);
  URT_GUARD_END(ctx)
}

int urt_shader_dispatch_rows(urt_context* ctx, int kernel, int groups_x, int groups_y, int groups_z, int first_group_row,
                             int row_stride) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  return do_dispatch(ctx, kernel, groups_x, groups_y, groups_z, first_group_row, row_stride);
  URT_GUARD_END(ctx)
}

/* ---- blits ---- */
int urt_blit_add(urt_context* ctx, urt_handle src, urt_handle dst, float sample) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  Texture* s = find_texture(ctx, src);
  Texture* d = find_texture(ctx, dst);
  if (!s || !d) return fail(ctx, URT_ERR_INVALID_HANDLE, "Blit: unknown texture handle");
  if (s->w != d->w || s->h != d->h) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "Blit: source and destination sizes differ");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  URT_GUARD_BEGIN
  d->other_writes = true;
  urt_context::Pending& B = ctx->pend;
  if (B.n > 0 && src == B.tex && dst != src && (const float4*)d->dev != B.S.sky) {
    // the source is a frame that has not been traced yet: the blend is deferred with it (flush_pending runs it in order)
    // (a full batch is submitted by the next dispatch or observer — the present of this frame, RM:819, may still follow)
    B.ops.push_back(PostOp{.kind = OpKind::BlendAdd, .frame = B.n - 1, .src = src, .dst = dst, .sample = sample});
    return URT_OK;
  }
  { int rc = flush_pending(ctx); if (rc) return rc; }
  URT_HIP(ctx, launch_blit_add(s->dev, d->dev, (size_t)s->w * s->h, sample, touch(ctx)));
  return URT_OK;
  URT_GUARD_END(ctx)
}

// AdditionShader blend with a per-pixel sample count (include/urt.h).  Deferred like urt_blit_add when src is the pending batch's Result
// texture (flush_pending fuses runs of them); otherwise the deferred frames are submitted and the blend is enqueued.
int urt_blit_add_history(urt_context* ctx, urt_handle src, urt_handle dst, urt_handle count, float max_history) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  Texture* s = find_texture(ctx, src);
  Texture* d = find_texture(ctx, dst);
  Texture* c = find_texture(ctx, count);
  if (!s || !d || !c) return fail(ctx, URT_ERR_INVALID_HANDLE, "blit_add_history: unknown texture handle");
  if (s->w != d->w || s->h != d->h || c->w != d->w || c->h != d->h)
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "blit_add_history: the textures differ in size");
  if (src == dst || count == src || count == dst) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "blit_add_history: src, dst and count must differ");
  if (dst == ctx->t_sky || count == ctx->t_sky)
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "blit_add_history: dst or count is the texture bound as _SkyboxTexture");
  if (!valid_max_history(max_history)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "blit_add_history: max_history must be 0 or >= 1");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  URT_GUARD_BEGIN
  d->other_writes = true;
  c->other_writes = true;
  urt_context::Pending& B = ctx->pend;
  if (B.n > 0 && src == B.tex && (const float4*)d->dev != B.S.sky && (const float4*)c->dev != B.S.sky) {
    B.ops.push_back(PostOp{.kind = OpKind::BlendHistory, .frame = B.n - 1, .src = src, .dst = dst, .count = count, .max_history = max_history});
    return URT_OK;
  }
  { int rc = flush_pending(ctx); if (rc) return rc; }
  URT_HIP(ctx, launch_blit_add_history(s->dev, d->dev, c->dev, (size_t)s->w * s->h, max_history, touch(ctx)));
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_blit(urt_context* ctx, urt_handle src, urt_handle dst) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  Texture* s = find_texture(ctx, src);
  Texture* d = find_texture(ctx, dst);
  if (!s || !d) return fail(ctx, URT_ERR_INVALID_HANDLE, "Blit: unknown texture handle");
  if (s->w != d->w || s->h != d->h) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "Blit: source and destination sizes differ");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  URT_GUARD_BEGIN
  urt_context::Pending& B = ctx->pend;
  if (B.n > 0 && dst != B.tex && dst != src && (const float4*)d->dev != B.S.sky) {
    // frames are deferred: the copy is queued behind them, in program order (the present of RM:819 — its source is the image
    // the deferred blends accumulate into).  flush_pending fuses it into the blend pass.
    d->other_writes = true;
    B.ops.push_back(PostOp{.kind = OpKind::Copy, .frame = B.n - 1, .src = src, .dst = dst});
    if (B.n >= B.limit) return flush_pending(ctx);        // the batch is full and its last frame is presented: go
    return URT_OK;
  }
  { int rc = flush_pending(ctx); if (rc) return rc; }
  d->other_writes = true;
  if (dst != src)
    URT_HIP(ctx, hipMemcpyAsync(d->dev, s->dev, (size_t)s->w * s->h * sizeof(float4), hipMemcpyDeviceToDevice, touch(ctx)));
  return URT_OK;
  URT_GUARD_END(ctx)
}

static int pack_impl(urt_context* ctx, urt_handle texture, int first_group_row, int row_stride, void* dense, bool to_dense,
                     uint64_t* out_bytes, bool rgb = false, float alpha = 0.0f) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  Texture* t = find_texture(ctx, texture);
  if (!t) return fail(ctx, URT_ERR_INVALID_HANDLE, "unknown texture handle");
  if (first_group_row < 0 || row_stride < 1) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "bad strip arguments");
  int n_strips = strip_count((t->h + 7) / 8, first_group_row, row_stride);
  if (out_bytes) *out_bytes = (uint64_t)n_strips * 8u * (uint64_t)t->w * (rgb ? 3 * sizeof(float) : sizeof(float4));
  if (!dense) return URT_OK;   // size query
  URT_HIP(ctx, hipSetDevice(ctx->device));
  URT_GUARD_BEGIN
  urt_context::Pending& B = ctx->pend;
  if (to_dense && B.n > 0) {     // reads an image that deferred work is still going to write: deferred with it, in order
    B.ops.push_back(PostOp{.kind = OpKind::PackRows, .frame = B.n - 1, .src = texture, .dense = dense,
                           .first_row = first_group_row, .row_stride = row_stride, .rgb = rgb});
    return URT_OK;
  }
  { int rc = flush_pending(ctx); if (rc) return rc; }
  if (!to_dense) t->other_writes = true;
  URT_GUARD_END(ctx)
  if (rgb) URT_HIP(ctx, launch_pack_rows_rgb(t->dev, (float*)dense, t->w, t->h, first_group_row, row_stride, n_strips, to_dense, alpha, touch(ctx)));
  else URT_HIP(ctx, launch_pack_rows(t->dev, (float4*)dense, t->w, t->h, first_group_row, row_stride, n_strips, to_dense, touch(ctx)));
  return URT_OK;
}

int urt_texture_pack_rows(urt_context* ctx, urt_handle texture, int first_group_row, int row_stride, void* device_dst,
                          uint64_t* out_bytes) {
  return pack_impl(ctx, texture, first_group_row, row_stride, device_dst, true, out_bytes);
}

static int unpack_on_impl(urt_context* ctx, urt_handle texture, int first_group_row, int row_stride, const void* device_src,
                          void* hip_stream, bool rgb, float alpha) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!device_src || !hip_stream) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "device_src / hip_stream is NULL");
  Texture* t = find_texture(ctx, texture);
  if (!t) return fail(ctx, URT_ERR_INVALID_HANDLE, "unknown texture handle");
  if (first_group_row < 0 || row_stride < 1) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "bad strip arguments");
  if (ctx->pend.n > 0) {                                  // never the case for a dedicated gather target
    bool touched = ctx->pend.tex == texture;
    for (const PostOp& q : ctx->pend.ops) touched = touched || q.touches(texture);
    if (touched) { int rc = flush_pending(ctx); if (rc) return rc; }
  }
  if (in_slab(ctx, *t)) { int rc = detach_from_slab(ctx, *t); if (rc) return rc; }
  int n_strips = strip_count((t->h + 7) / 8, first_group_row, row_stride);
  t->other_writes = true;
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (rgb) URT_HIP(ctx, launch_pack_rows_rgb(t->dev, (float*)const_cast<void*>(device_src), t->w, t->h, first_group_row, row_stride, n_strips, false,
                                            alpha, (hipStream_t)hip_stream));
  else URT_HIP(ctx, launch_pack_rows(t->dev, (float4*)const_cast<void*>(device_src), t->w, t->h, first_group_row, row_stride, n_strips, false,
                                     (hipStream_t)hip_stream));
  return URT_OK;
}

int urt_texture_unpack_rows_on(urt_context* ctx, urt_handle texture, int first_group_row, int row_stride, const void* device_src,
                               void* hip_stream) {
  return unpack_on_impl(ctx, texture, first_group_row, row_stride, device_src, hip_stream, false, 0.0f);
}

int urt_texture_pack_rows_rgb(urt_context* ctx, urt_handle texture, int first_group_row, int row_stride, void* device_dst,
                              uint64_t* out_bytes) {
  return pack_impl(ctx, texture, first_group_row, row_stride, device_dst, true, out_bytes, true);
}

int urt_texture_unpack_rows_rgb(urt_context* ctx, urt_handle texture, int first_group_row, int row_stride, const void* device_src,
                                float alpha, void* hip_stream) {
  if (ctx && !device_src) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "device_src is NULL");
  if (hip_stream) return unpack_on_impl(ctx, texture, first_group_row, row_stride, device_src, hip_stream, true, alpha);
  return pack_impl(ctx, texture, first_group_row, row_stride, const_cast<void*>(device_src), false, nullptr, true, alpha);
}

int urt_texture_unpack_rows(urt_context* ctx, urt_handle texture, int first_group_row, int row_stride, const void* device_src) {
  if (ctx && !device_src) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "device_src is NULL");
  return pack_impl(ctx, texture, first_group_row, row_stride, const_cast<void*>(device_src), false, nullptr);
}

/* ---- options ---- */
namespace {
// One row per option of urt_set_option.  A value must lie in [lo, hi] and pass `ok` (if any), else the call fails with `msg`.
// kBool: any value, stored as 0 / 1.  kStale: the next dispatch prepares the scene from scratch.  kFlushAgain: the deferred frames are
// submitted once more before the value is stored.  kOnChange: kStale / kFlushAgain act only when the value differs from the stored one.
enum : unsigned { kBool = 1, kStale = 2, kFlushAgain = 4, kOnChange = 8 };
struct OptionRow { const char* name; int urt_context::Options::* field; int lo, hi; const char* msg; unsigned flags; bool (*ok)(int); };
using O = urt_context::Options;
const OptionRow kOptions[] = {
  {"blas_builder", &O::blas_builder, -1, 3, "blas_builder must be -1 (auto), 0 (host SAH), 1 (GPU LBVH), 2 (GPU LBVH built top-down within a depth budget) or 3 (binned SAH on the GPU)", kStale | kOnChange, nullptr},
  {"frames_per_launch", &O::frames_per_launch, 0, kMaxFramesPerLaunch, "frames_per_launch must be in [0, 64] (0 = auto)", 0, nullptr},
  {"count_stats", &O::count_stats, INT_MIN, INT_MAX, "", kBool, nullptr},
  {"time_dispatch", &O::time_dispatch, INT_MIN, INT_MAX, "", kBool, nullptr},
  {"kernel_mode", &O::kernel_mode, 0, 5, "kernel_mode must be 0..5", 0, nullptr},
  {"block_threads", &O::block_threads, 64, 256, "block_threads must be 64, 128 or 256", 0, [](int v) { return v == 64 || v == 128 || v == 256; }},
  {"blas_leaf_max", nullptr /* process-wide: set_blas_leaf_max */, 1, 8, "blas_leaf_max must be in [1, 8]", kStale, nullptr},
  {"blas_min", &O::blas_min, 0, 256, "blas_min must be in [0, 256] (0 = auto; kernel_mode 5 counts the waiting rays of a workgroup)", 0, nullptr},
  {"blas_exit", &O::blas_exit, 0, 64, "blas_exit must be in [0, 64] (0 = auto)", 0, nullptr},
  {"refill_min", &O::refill_min, 1, 64, "refill_min must be in [1, 64]", 0, nullptr},
  {"waves_per_cu", &O::waves_per_cu, 0, 32, "waves_per_cu must be in [0, 32] (0 = auto)", 0, nullptr},
  {"sched_block", &O::sched_block, 0, 256, "sched_block must be 0 (auto), 64 or 256", 0, [](int v) { return v == 0 || v == 64 || v == 256; }},
  {"stack_pad", &O::stack_pad, 0, 96, "stack_pad must be in [0, 96]", 0, nullptr},
  {"radiance_persist", &O::radiance_persist, -1, 1, "radiance_persist must be -1 (auto), 0 or 1", 0, nullptr},
  {"shade_min", &O::shade_min, 1, 64, "shade_min must be in [1, 64]", 0, nullptr},
  {"front_list", &O::front_list, -1, 2, "front_list must be -1 (auto), 0, 1 or 2", 0, nullptr},
  {"shade_split", &O::shade_split, -1, 1, "shade_split must be -1 (auto), 0 or 1", 0, nullptr},
  {"serve_refill", &O::serve_refill, 1, 64, "serve_refill must be in [1, 64]", 0, nullptr},
  {"sky_min", &O::sky_min, 1, 64, "sky_min must be in [1, 64]", 0, nullptr},
  {"tile_order", &O::tile_order, -1, 1, "tile_order must be -1 (auto), 0 or 1", 0, nullptr},
  {"lds_tlas", &O::lds_tlas, INT_MIN, INT_MAX, "", kBool, nullptr},
  {"top_front", &O::top_front, -1, 1, "top_front must be -1 (auto), 0 or 1", 0, nullptr},
  {"top_nodes", &O::top_nodes, -1, kTopOrderNodes, "top_nodes must be in [0, 256], or -1 (auto)", 0, nullptr},
  {"pool_k", &O::pool_k, 1, 4, "pool_k must be in [1, 4]", 0, nullptr},
  {"pool_refill", &O::pool_refill, 1, 256, "pool_refill must be in [1, 256]", 0, nullptr},
  {"pool_blas_min", &O::pool_blas_min, 1, 256, "pool_blas_min must be in [1, 256]", 0, nullptr},
  {"pool_blas_exit", &O::pool_blas_exit, 1, 64, "pool_blas_exit must be in [1, 64]", 0, nullptr},
  {"pool_other_min", &O::pool_other_min, 1, 64, "pool_other_min must be in [1, 64]", 0, nullptr},
  {"pool_inloop", &O::pool_inloop, 1, 64, "pool_inloop must be in [1, 64]", 0, nullptr},
  {"frame_group", &O::frame_group, 1, kMaxFramesPerLaunch, "frame_group must be in [1, 64]", 0, nullptr},
  {"work_shards", &O::work_shards, 1, (int)kWorkShards, "work_shards must be a power of two in [1, 64]", 0, [](int v) { return (v & (v - 1)) == 0; }},
  {"qnodes", &O::qnodes, -1, 1, "qnodes must be -1 (auto), 0 or 1", kStale, nullptr},
  {"lbvh_slack", &O::lbvh_slack, 0, 16, "lbvh_slack must be 0..16", kStale | kOnChange, nullptr},
  {"overlap_launches", &O::overlap_launches, 0, 2, "overlap_launches must be 0 (off), 1 (auto) or 2 (always)", kFlushAgain, nullptr},
  {"blas_cones", &O::blas_cones, -1, 1, "blas_cones must be -1 (auto), 0 or 1", kStale | kOnChange, nullptr},
  {"tile_entry", &O::tile_entry, -1, 1, "tile_entry must be -1 (auto), 0 or 1", 0, nullptr},
  {"front_cull", &O::front_cull, 0, 1, "front_cull must be 0 or 1", kFlushAgain | kStale | kOnChange, nullptr},
  {"front_fuse", &O::front_fuse, -1, 1, "front_fuse must be -1 (auto), 0 or 1", kOnChange, nullptr},
  {"handout", &O::handout, -1, 1, "handout must be -1 (auto), 0 or 1", 0, nullptr},
  {"refit", &O::refit, INT_MIN, INT_MAX, "", kBool | kStale, nullptr},
  {"refit_vertices", &O::refit_vertices, INT_MIN, INT_MAX, "", kBool, nullptr},
  {"prepare_device", &O::prepare_device, INT_MIN, INT_MAX, "", kBool | kStale, nullptr},
  {"refit_rebuild_pct", &O::refit_rebuild_pct, 0, INT_MAX, "refit_rebuild_pct must be 0 (never rebuild) or greater than 100", 0, [](int v) { return v == 0 || v > 100; }},
  {"watchdog_cap", &O::watchdog_cap, 0, INT_MAX, "watchdog_cap must be >= 0 (0 = auto)", 0, nullptr},
  {"xcd_run", &O::xcd_run, 0, 4096, "xcd_run must be in [0, 4096] (0 = auto)", 0, nullptr},
};
}  // namespace

int urt_set_option(urt_context* ctx, const char* name, int value) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!name) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "option name is NULL");
  { (void)hipSetDevice(ctx->device); int rc = flush_pending(ctx); if (rc) return rc; }   // deferred frames run with the options they were dispatched under
  const OptionRow* r = std::find_if(std::begin(kOptions), std::end(kOptions), [&](const OptionRow& o) { return std::strcmp(name, o.name) == 0; });
  if (r == std::end(kOptions)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, std::string("unknown option ") + name);
  if (value < r->lo || value > r->hi || (r->ok && !r->ok(value))) return fail(ctx, URT_ERR_INVALID_ARGUMENT, r->msg);
  if (r->flags & kBool) value = value ? 1 : 0;
  const bool act = !(r->flags & kOnChange) || ctx->opt.*r->field != value;
  if ((r->flags & kFlushAgain) && act) { int rc = flush_pending(ctx); if (rc) return rc; }
  if ((r->flags & kStale) && act) { ctx->scene_dirty = true; ctx->dirty_full = true; }
  if (r->field) ctx->opt.*r->field = value; else set_blas_leaf_max(value);
  return URT_OK;
}

int urt_get_counters(urt_context* ctx, urt_counters* out) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!out) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "out is NULL");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  { int rc = flush_pending(ctx); if (rc) return rc; }
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  resolve_timing(ctx);
  std::vector<DevCounters> shards(kCounterShards);
  URT_HIP(ctx, hipMemcpy(shards.data(), ctx->d_counters.get(), sizeof(DevCounters) * kCounterShards, hipMemcpyDeviceToHost));
  std::memset(out, 0, sizeof *out);
  for (const DevCounters& dc : shards) {
    out->rays += dc.rays; out->tlas_nodes += dc.tlas_nodes; out->blas_nodes += dc.blas_nodes; out->tri_tests += dc.tri_tests;
    out->sphere_tests += dc.sphere_tests; out->hit_tri += dc.hit_tri; out->hit_sphere += dc.hit_sphere;
    out->hit_ground += dc.hit_ground; out->hit_sky += dc.hit_sky;
    out->watchdog_trips += (uint32_t)dc.watchdog;
  }
  out->pixels = ctx->pixels_dispatched;
  out->dispatches = ctx->dispatches;
  out->launches = ctx->launches;
  out->trace_ms = ctx->trace_ms;
  return URT_OK;
}

int urt_reset_counters(urt_context* ctx) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  { int rc = flush_pending(ctx); if (rc) return rc; }
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  resolve_timing(ctx);
  URT_HIP(ctx, hipMemset(ctx->d_counters.get(), 0, sizeof(DevCounters) * kCounterShards));
  if (ctx->h_trip_flag) __atomic_store_n(ctx->h_trip_flag.get(), 0u, __ATOMIC_RELEASE);
  ctx->dispatches = 0;
  ctx->launches = 0;
  ctx->pixels_dispatched = 0;
  ctx->trace_ms = 0;
  return URT_OK;
}

#ifdef URT_STAMPS
/* diagnostic builds only: per-wave (start, pool-exhausted, end, iters<<32|fetches) of the last persistent launch */
__attribute__((visibility("default"))) int urt_debug_read_stamps(urt_context* ctx, unsigned long long* out, int n_waves) {
  (void)hipStreamSynchronize(touch(ctx));
  hipError_t e = hipMemcpy(out, (char*)ctx->d_next.get() + urt_context::kStampOffset, (size_t)n_waves * sizeof(unsigned long long), hipMemcpyDeviceToHost);   // n_waves = number of u64 words
  (void)hipMemset((char*)ctx->d_next.get() + urt_context::kStampOffset, 0, urt_context::kStampBytes);
  return (int)e;
}
#endif

/* kernel_mode 5 with count_stats: visits of the traversal service, its trips, active lanes summed over the trips, claim rounds,
   rays claimed, rays suspended — summed since the last urt_reset_counters */
int urt_debug_serve_stats(urt_context* ctx, unsigned long long* out6) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!out6) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "out6 is NULL");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  { int rc = flush_pending(ctx); if (rc) return rc; }
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  std::vector<DevCounters> shards(kCounterShards);
  URT_HIP(ctx, hipMemcpy(shards.data(), ctx->d_counters.get(), sizeof(DevCounters) * kCounterShards, hipMemcpyDeviceToHost));
  for (int q = 0; q < 6; q++) out6[q] = 0;
  for (const DevCounters& dc : shards) for (int q = 0; q < 6; q++) out6[q] += dc.serve[q];
  return URT_OK;
}

/* ---- introspection ---- */
int urt_debug_build_blas(const void* mesh_objects, int n_meshes, const float* vertices, int n_vertices, const int32_t* indices,
                         int n_indices, int* out_n_nodes, int* out_n_tris, int* out_max_depth) {
  URT_GUARD_BEGIN
  if (n_meshes < 0 || (n_meshes > 0 && !mesh_objects)) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "mesh_objects is NULL");
  std::string err;
  if (!build_blas((const uint8_t*)mesh_objects, n_meshes, vertices, n_vertices, indices, n_indices, nullptr, 0, g_debug_blas, err))
    return fail(nullptr, URT_ERR_SCENE, err);
  if (out_n_nodes) *out_n_nodes = (int)(g_debug_blas.nodes.size() / kBlasNodeFloats);
  if (out_n_tris) *out_n_tris = (int)g_debug_blas.tri_slot.size();
  if (out_max_depth) *out_max_depth = g_debug_blas.max_depth;
  return URT_OK;
  URT_GUARD_END(nullptr)
}

int urt_debug_blas_cache_stats(urt_context* ctx, uint64_t* out_reused, uint64_t* out_built) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  std::lock_guard<std::mutex> g(ctx->blas_cache.lock);
  if (out_reused) *out_reused = ctx->blas_cache.hits;
  if (out_built) *out_built = ctx->blas_cache.builds;
  return URT_OK;
}

/* The masked-walk table the default kernel derives from a mesh heap of <= 31 nodes (build_walk_table above), for host-side tests:
   out = (20 + 2 * n_eval) * 4 words; returns the number of words written through out_words, 0 when the heap does not qualify. */
int urt_debug_build_walk_table(const urt_BVHNode* heap, int n_nodes, int n_meshes, const int32_t* mesh_root, const int32_t* small_first,
                               float* out, int capacity_words, int* out_words) {
  if (out_words) *out_words = 0;
  if (n_nodes < 0 || (n_nodes > 0 && !heap) || n_meshes < 0 || (n_meshes > 0 && !mesh_root)) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "urt_debug_build_walk_table: bad arguments");
  URT_GUARD_BEGIN
  Buffer b; b.count = n_nodes; b.stride = URT_STRIDE_BVHNODE; b.has_data = true;
  b.host.resize((size_t)n_nodes * URT_STRIDE_BVHNODE);
  if (n_nodes > 0) std::memcpy(b.host.data(), heap, b.host.size());
  std::vector<int32_t> roots(mesh_root, mesh_root + n_meshes), sf;
  if (small_first) sf.assign(small_first, small_first + n_meshes);
  std::vector<float> t;
  if (!build_walk_table(n_nodes > 0 ? &b : nullptr, n_meshes, roots, sf, t)) return URT_OK;
  if ((int)t.size() > capacity_words || !out) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "urt_debug_build_walk_table: output buffer too small");
  std::memcpy(out, t.data(), t.size() * sizeof(float));
  if (out_words) *out_words = (int)t.size();
  return URT_OK;
  URT_GUARD_END(nullptr)
}

int urt_debug_refit_stats(urt_context* ctx, uint64_t* out_refitted_meshes, uint64_t* out_incremental_preparations) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (out_refitted_meshes) *out_refitted_meshes = ctx->refitted_meshes;
  if (out_incremental_preparations) *out_incremental_preparations = ctx->incremental_preps;
  return URT_OK;
}

int urt_debug_deform_stats(urt_context* ctx, uint64_t out6[6]) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!out6) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "out6 is NULL");
  uint32_t ratio_bits;
  std::memcpy(&ratio_bits, &ctx->last_cost_ratio, 4);
  out6[0] = ctx->deformed_meshes; out6[1] = ctx->renormed_meshes; out6[2] = ctx->deform_bytes; out6[3] = ctx->forced_rebuilds;
  out6[4] = ratio_bits; out6[5] = 0;
  return URT_OK;
}

int urt_debug_scene_cost(urt_context* ctx, float* out, int n_meshes) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (n_meshes < 0 || (n_meshes > 0 && !out)) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "urt_debug_scene_cost: out is NULL or n_meshes negative");
  URT_GUARD_BEGIN
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = current_scene(ctx)) return rc;
  if (n_meshes != ctx->scene.ds.n_meshes) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "urt_debug_scene_cost: n_meshes is not the scene's number of MeshObjects");
  std::vector<float> now, base;
  if (int rc = scene_cost(ctx, now, base)) return rc;
  for (int m = 0; m < n_meshes; m++) { out[2 * m] = now[(size_t)m]; out[2 * m + 1] = base[(size_t)m]; }
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_debug_live_resources(uint64_t out4[4]) {
  if (!out4) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "out4 is NULL");
  out4[0] = g_live.device_bytes; out4[1] = g_live.pinned_bytes; out4[2] = g_live.events; out4[3] = g_live.streams;
  return URT_OK;
}

int urt_debug_launch_info(urt_context* ctx, urt_launch_info* out) {
  if (!ctx || !out) return URT_ERR_INVALID_ARGUMENT;
  int rc = flush_pending(ctx); if (rc) return rc;          // "the last launch" includes the frames still deferred
  *out = ctx->last_launch;
  out->slab_frames = ctx->slab_frames; out->slab_frames_max = ctx->slab_frames_max; out->slab_out_of_memory = ctx->slab_oom_stride != 0 ? 1 : 0;
  out->blas_builder = ctx->last_builder;
  out->overlapped_launches = (int)std::min<uint64_t>(ctx->overlapped_launches, 0x7fffffff);
  return URT_OK;
}

int urt_debug_scene_info(urt_context* ctx, int* out_n_nodes, int* out_n_tris, int* out_max_depth, float* out_prepare_ms) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = current_scene(ctx)) return rc;
  if (out_n_nodes) *out_n_nodes = ctx->scene.n_blas_nodes;
  if (out_n_tris) *out_n_tris = ctx->scene.n_scene_tris;
  if (out_max_depth) *out_max_depth = ctx->scene.scene_max_depth;
  if (out_prepare_ms) *out_prepare_ms = ctx->last_prepare_ms;
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_debug_scene_vertex_spans(urt_context* ctx, int32_t* out_lo, int32_t* out_hi, int n_meshes) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (n_meshes < 0 || (n_meshes > 0 && (!out_lo || !out_hi))) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "urt_debug_scene_vertex_spans: out_lo / out_hi is NULL or n_meshes negative");
  URT_GUARD_BEGIN
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = current_scene(ctx)) return rc;
  if (n_meshes != ctx->scene.ds.n_meshes) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "urt_debug_scene_vertex_spans: n_meshes is not the scene's number of MeshObjects");
  const bool kept = ctx->scene.h_vert_lo.size() == (size_t)n_meshes && ctx->scene.h_vert_hi.size() == (size_t)n_meshes;
  for (int m = 0; m < n_meshes; m++) {
    out_lo[m] = kept ? ctx->scene.h_vert_lo[(size_t)m] : INT32_MAX;
    out_hi[m] = kept ? ctx->scene.h_vert_hi[(size_t)m] : -1;
  }
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_debug_prepare_stats(urt_context* ctx, uint64_t out4[4]) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!out4) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "out4 is NULL");
  uint32_t ms_bits;
  std::memcpy(&ms_bits, &ctx->last_span_ms, 4);
  out4[0] = ctx->full_preps; out4[1] = ctx->device_preps; out4[2] = (uint64_t)kSpanChunk; out4[3] = ms_bits;
  return URT_OK;
}

int urt_debug_read_scene_blas(urt_context* ctx, float* nodes, int32_t* tri_index, int32_t* mesh_root) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = current_scene(ctx)) return rc;
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  const DevScene& S = ctx->scene.ds;
  if (nodes && ctx->scene.n_blas_nodes > 0) URT_HIP(ctx, hipMemcpy(nodes, S.blas_nodes, (size_t)ctx->scene.n_blas_nodes * kBlasNodeFloats * sizeof(float), hipMemcpyDeviceToHost));
  if (mesh_root && S.n_meshes > 0) URT_HIP(ctx, hipMemcpy(mesh_root, S.mesh_root, (size_t)S.n_meshes * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (tri_index && ctx->scene.n_scene_tris > 0) {
    std::vector<float> tv((size_t)ctx->scene.n_scene_tris * 12);
    URT_HIP(ctx, hipMemcpy(tv.data(), S.tri_verts, tv.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int k = 0; k < ctx->scene.n_scene_tris; k++) std::memcpy(&tri_index[k], &tv[(size_t)k * 12 + 3], 4);     // index slot kept in v0.w
  }
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_debug_read_scene_qnodes(urt_context* ctx, float* out, int* out_n_nodes, int* out_in_use) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = current_scene(ctx)) return rc;
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  // qbuf exists (and is current) only while the option is on: it is derived after every build and refit (rederive_nodes)
  const bool have = ctx->opt.qnodes != 0 && ctx->scene.qbuf && ctx->scene.n_blas_nodes > 0;
  if (out_n_nodes) *out_n_nodes = have ? ctx->scene.n_blas_nodes : 0;
  if (out_in_use) *out_in_use = ctx->scene.ds.blas_qnodes != nullptr ? 1 : 0;
  if (out && have) URT_HIP(ctx, hipMemcpy(out, ctx->scene.qbuf, (2 + 2 * (size_t)ctx->scene.n_blas_nodes) * sizeof(float4), hipMemcpyDeviceToHost));
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_debug_read_scene_cones(urt_context* ctx, uint32_t* words, float* tri_edges, int* out_in_use) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = current_scene(ctx)) return rc;
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  const DevScene& S = ctx->scene.ds;
  const size_t nn = (size_t)std::max(0, ctx->scene.n_blas_nodes), nt = (size_t)std::max(0, ctx->scene.n_scene_tris);
  if (out_in_use) *out_in_use = ctx->scene.cones_in_use ? 1 : 0;
  if (words && nn > 0 && S.blas_cnodes) {
    std::vector<float> cn(nn * 16);
    URT_HIP(ctx, hipMemcpy(cn.data(), S.blas_cnodes, cn.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t n = 0; n < nn; n++) std::memcpy(&words[2 * n], &cn[n * 16 + 14], 8);
  }
  if (tri_edges && nt > 0) {
    std::vector<float> tv(nt * 12);
    URT_HIP(ctx, hipMemcpy(tv.data(), S.tri_verts, tv.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < nt; k++) { std::memcpy(&tri_edges[6 * k], &tv[k * 12 + 4], 12); std::memcpy(&tri_edges[6 * k + 3], &tv[k * 12 + 8], 12); }
  }
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_debug_read_tile_entry(urt_context* ctx, int32_t* out, uint64_t capacity_words, int* out_tiles_x, int* out_tiles_y, int* out_k, uint64_t* out_builds) {
  if (!ctx) return fail(nullptr, URT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  URT_GUARD_BEGIN
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = flush_pending(ctx)) return rc;
  const bool have = ctx->te_valid && ctx->te_table;
  const int tx = have ? (ctx->te_key.width + 7) / 8 : 0, ty = have ? (ctx->te_key.height + 7) / 8 : 0;
  if (out_tiles_x) *out_tiles_x = tx;
  if (out_tiles_y) *out_tiles_y = ty;
  if (out_k) *out_k = have ? kTileEntryK : 0;
  if (out_builds) *out_builds = ctx->te_builds;
  if (out && have) {
    URT_HIP(ctx, hipEventSynchronize(ctx->te_ready.get()));
    const uint64_t words = std::min<uint64_t>(capacity_words, (uint64_t)tx * (uint64_t)ty * kTileEntryK);
    if (words) URT_HIP(ctx, hipMemcpy(out, ctx->te_table.get(), words * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return URT_OK;
  URT_GUARD_END(ctx)
}

int urt_debug_get_blas(float* nodes, int32_t* tri_index, int32_t* mesh_root, int32_t* mesh_first_tri) {
  const BlasResult& b = g_debug_blas;
  if (nodes && !b.nodes.empty()) std::memcpy(nodes, b.nodes.data(), b.nodes.size() * sizeof(float));
  if (tri_index && !b.tri_slot.empty()) std::memcpy(tri_index, b.tri_slot.data(), b.tri_slot.size() * sizeof(int32_t));
  if (mesh_root && !b.mesh_root.empty()) std::memcpy(mesh_root, b.mesh_root.data(), b.mesh_root.size() * sizeof(int32_t));
  if (mesh_first_tri && !b.mesh_first_tri.empty()) std::memcpy(mesh_first_tri, b.mesh_first_tri.data(), b.mesh_first_tri.size() * sizeof(int32_t));
  return URT_OK;
}

}  // extern "C"

// ---- internal accessors for group.cpp (not part of the C ABI) ----------------------------------------------------------
namespace urtd {
hipStream_t context_stream(urt_context* ctx) { return touch(ctx); }   // (csrc/group.cpp enqueues gathers and blits on it)
int context_device(urt_context* ctx) { return ctx->device; }
int context_pending_frames(urt_context* ctx) { return ctx->pend.n; }
}  // namespace urtd