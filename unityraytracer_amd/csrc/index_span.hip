// index_span.hip — per MeshObject the smallest and the largest vertex its index range names, from the device copy of _Indices.
// A full preparation that takes its geometry from device memory (option "prepare_device", scene_prep.cpp) has no host copy of _Indices to
// scan; the in-place update of deformed meshes (prepare_incremental) needs these spans.
//   k_span_init   lo_hi = (INT32_MAX, -1) per MeshObject
//   k_spans       one wave per (MeshObject, chunk) item of the host's table: a one-pass streaming read of the item's indices
#include "index_span.h"

#include <algorithm>
#include <climits>

namespace urtd {
namespace {

constexpr int kSpanBlock = 256;                              // 4 waves = 4 items per workgroup

__global__ __launch_bounds__(kSpanBlock) void k_span_init(int32_t* __restrict__ lo_hi, int n_meshes) {
  const int m = (int)(blockIdx.x * kSpanBlock + threadIdx.x);
  if (m < n_meshes) { lo_hi[2 * m] = INT_MAX; lo_hi[2 * m + 1] = -1; }
}

__device__ inline void join(int& lo, int& hi, int v) { lo = min(lo, v); hi = max(hi, v); }

// The item's range starts at any index slot, so it is read as up to three leading words, 16-byte vectors, and up to three trailing words:
// nothing outside [first, first + count) is touched.  Each lane reduces what it read, the wave reduces by shuffles, and lane 0 joins the
// MeshObject's words — with an atomic only when a plain read says the word would change: the words move one way only, so a stale read
// can cost an atomic that changes nothing and never one that was needed.
__global__ __launch_bounds__(kSpanBlock) void k_spans(const int32_t* __restrict__ indices, const SpanItem* __restrict__ items, int n_items,
                                                      int32_t* __restrict__ lo_hi) {
  const int lane = (int)(threadIdx.x & 63u);
  const int item = (int)(blockIdx.x * (kSpanBlock / 64) + (threadIdx.x >> 6));
  if (item >= n_items) return;                               // (wave-uniform)
  const SpanItem it = items[item];
  const int32_t* p = indices + (size_t)it.first;
  const int head = min(it.count, (int)((0u - (unsigned int)((uintptr_t)p >> 2)) & 3u));
  const int n_vec = (it.count - head) >> 2, tail = (it.count - head) & 3;
  const int4* body = (const int4*)(p + head);
  int lo = INT_MAX, hi = INT_MIN;
#pragma unroll 4
  for (int k = lane; k < n_vec; k += 64) {
    const int4 v = body[k];
    join(lo, hi, v.x); join(lo, hi, v.y); join(lo, hi, v.z); join(lo, hi, v.w);
  }
  if (lane < head) join(lo, hi, p[lane]);
  if (lane < tail) join(lo, hi, p[head + 4 * n_vec + lane]);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) { lo = min(lo, __shfl_xor(lo, s, 64)); hi = max(hi, __shfl_xor(hi, s, 64)); }
  if (lane == 0) {
    int32_t* w = lo_hi + 2 * (size_t)it.mesh;
    if (lo < __atomic_load_n(w, __ATOMIC_RELAXED)) atomicMin(w, lo);
    if (hi > __atomic_load_n(w + 1, __ATOMIC_RELAXED)) atomicMax(w + 1, hi);
  }
}

}  // namespace

bool span_items(const int32_t* offsets, const int32_t* counts, int n_meshes, int n_indices, std::vector<SpanItem>& out) {
  out.clear();
  for (int m = 0; m < n_meshes; m++) {
    const long off = offsets[m], cnt = counts[m];
    if (off < 0 || cnt < 0 || off + cnt > (long)n_indices) { out.clear(); return false; }
    const long scanned = cnt / 3 * 3;
    for (long at = 0; at < scanned; at += kSpanChunk)
      out.push_back(SpanItem{m, (int32_t)(off + at), (int32_t)std::min<long>(kSpanChunk, scanned - at), 0});
  }
  return true;
}

hipError_t index_spans(const int32_t* indices, const SpanItem* items, int n_items, int32_t* lo_hi, int n_meshes, hipStream_t st) {
  if (n_meshes <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_span_init, dim3((unsigned int)((n_meshes + kSpanBlock - 1) / kSpanBlock)), dim3(kSpanBlock), 0, st, lo_hi, n_meshes);
  if (n_items > 0)
    hipLaunchKernelGGL(k_spans, dim3((unsigned int)((n_items + kSpanBlock / 64 - 1) / (kSpanBlock / 64))), dim3(kSpanBlock), 0, st, indices, items, n_items, lo_hi);
  return hipGetLastError();
}

}  // namespace urtd
