// skin.hip — what a host that animates on the GPU needs in front of the refit (scene_prep.cpp prepare_incremental):
//   k_skin     linear blend skinning of a range of vertices (and normals) into the device mirrors of two ComputeBuffers
//   k_bounds   component-wise min / max over the finite elements of a range of a stride-12 buffer
// The arithmetic of k_skin is NORMATIVE (include/urt.h urt_skin_vertices; tests/skin_ref.py restates it in numpy): float32, one
// rounding per operation, evaluated as written, no fma but the two of urt_math.h's dot().  Built with -ffp-contract=off like every
// normative kernel.
#include "skin.h"

#include <algorithm>

#include "../../include/urt_math.h"
#include "bounds_device.h"

namespace {

using namespace urt;
using urtd::Bounds;
using urtd::empty_bounds;
using urtd::join;
using urtd::kBoundsWords;
using urtd::reduce_and_store;
using urtd::kSkinBlock;

// One bone's contribution to a vertex: t = w * (A P + b), u = w * (A N); a[12] = three columns of A, then b.
template <bool kNormals>
__device__ __forceinline__ void skin_term(const float* __restrict__ a, float w, v3 P, v3 N, v3& t, v3& u) {
  const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7], a8 = a[8];
  t.x = w * (((a0 * P.x + a3 * P.y) + a6 * P.z) + a[9]);
  t.y = w * (((a1 * P.x + a4 * P.y) + a7 * P.z) + a[10]);
  t.z = w * (((a2 * P.x + a5 * P.y) + a8 * P.z) + a[11]);
  if (kNormals) {
    u.x = w * ((a0 * N.x + a3 * N.y) + a6 * N.z);
    u.y = w * ((a1 * N.x + a4 * N.y) + a7 * N.z);
    u.z = w * ((a2 * N.x + a5 * N.y) + a8 * N.z);
  }
}

// One vertex per lane, kSkinBlock vertices per workgroup.  The 12-byte elements are not read per lane: the workgroup's vertices are a
// contiguous span of 3 * kSkinBlock floats, which the lanes read (and, for the results, write) dword by dword in three passes, so every
// wave access covers whole cache lines; the span is turned by 90 degrees in LDS (stride 3 dwords: conflict-free).  kLdsBones: the bone
// table is staged in LDS (urtd::kSkinLdsBones), else every live term gathers its 48 bytes from global memory.
// block_first = first + blockIdx.x * kSkinBlock is the block's first element, in_block the number of its elements that lie in the range:
// only the last block is ragged, whatever `first` is.
template <bool kNormals, bool kLdsBones>
__global__ __launch_bounds__(kSkinBlock) void k_skin(const float* __restrict__ rest_v, const float* __restrict__ rest_n,
                                                     const int4* __restrict__ bone_idx, const float4* __restrict__ bone_wgt,
                                                     const float* __restrict__ bones, int n_bones, int first, int count,
                                                     float* __restrict__ dst_v, float* __restrict__ dst_n) {
  extern __shared__ float s_bones[];                       // 12 * n_bones floats when kLdsBones
  __shared__ float s_p[3 * kSkinBlock];
  __shared__ float s_n[kNormals ? 3 * kSkinBlock : 1];
  const int tid = (int)threadIdx.x;
  const long long block_first = (long long)first + (long long)blockIdx.x * kSkinBlock;
  const long long left = (long long)first + (long long)count - block_first;
  const int in_block = left < (long long)kSkinBlock ? (int)left : kSkinBlock;      // >= 1: the grid is ceil(count / kSkinBlock)
  const size_t base = (size_t)block_first * 3;
  const int span = 3 * in_block;
  for (int k = tid; k < span; k += kSkinBlock) {
    s_p[k] = rest_v[base + (size_t)k];
    if (kNormals) s_n[k] = rest_n[base + (size_t)k];
  }
  if (kLdsBones)
    for (int k = tid; k < 12 * n_bones; k += kSkinBlock) s_bones[k] = bones[k];
  __syncthreads();
  v3 pos = mk3(0.0f, 0.0f, 0.0f), nrm = mk3(0.0f, 0.0f, 0.0f);
  if (tid < in_block) {
    const v3 P = mk3(s_p[3 * tid], s_p[3 * tid + 1], s_p[3 * tid + 2]);
    const v3 N = kNormals ? mk3(s_n[3 * tid], s_n[3 * tid + 1], s_n[3 * tid + 2]) : mk3(0.0f, 0.0f, 0.0f);
    const int4 j4 = bone_idx[(size_t)block_first + (size_t)tid];
    const float4 w4 = bone_wgt[(size_t)block_first + (size_t)tid];
    const int j[4] = {j4.x, j4.y, j4.z, j4.w};
    const float w[4] = {w4.x, w4.y, w4.z, w4.w};
    v3 t[4], u[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      t[k] = mk3(0.0f, 0.0f, 0.0f); u[k] = mk3(0.0f, 0.0f, 0.0f);
      if (w[k] != 0.0f && j[k] >= 0 && j[k] < n_bones) {                           // live (a NaN weight is): else + 0, and the bone is not read
        const float* a = kLdsBones ? s_bones + 12 * j[k] : bones + 12 * (size_t)j[k];
        skin_term<kNormals>(a, w[k], P, N, t[k], u[k]);
      }
    }
    pos = ((t[0] + t[1]) + t[2]) + t[3];
    if (kNormals) {
      nrm = ((u[0] + u[1]) + u[2]) + u[3];
      const float l2 = dot(nrm, nrm);
      if (l2 > 0.0f && l2 < __builtin_inff()) nrm = normalize(nrm);
    }
  }
  __syncthreads();                                         // every lane has read its rest pose: the span now carries the results
  if (tid < in_block) {
    s_p[3 * tid] = pos.x; s_p[3 * tid + 1] = pos.y; s_p[3 * tid + 2] = pos.z;
    if (kNormals) { s_n[3 * tid] = nrm.x; s_n[3 * tid + 1] = nrm.y; s_n[3 * tid + 2] = nrm.z; }
  }
  __syncthreads();
  for (int k = tid; k < span; k += kSkinBlock) {
    dst_v[base + (size_t)k] = s_p[k];
    if (kNormals) dst_n[base + (size_t)k] = s_n[k];
  }
}

// First pass: the elements first .. first + count - 1 of a stride-12 buffer, grid-strided; an element counts when its three components are
// finite.  One partial per workgroup; no workgroup waits for another and nothing is combined with atomics.
__global__ __launch_bounds__(256) void k_bounds(const float* __restrict__ v, int first, int count, float* __restrict__ partial) {
  Bounds b = empty_bounds();
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < (long long)count; i += (long long)gridDim.x * 256) {
    const size_t at = ((size_t)first + (size_t)i) * 3;
    const float p[3] = {v[at], v[at + 1], v[at + 2]};
    const bool finite = (p[0] - p[0] == 0.0f) && (p[1] - p[1] == 0.0f) && (p[2] - p[2] == 0.0f);
    if (finite) join(b, p, p, 1u);
  }
  reduce_and_store(b, partial + (size_t)blockIdx.x * kBoundsWords);
}

// Second pass, one workgroup: the union of the partials.
__global__ __launch_bounds__(256) void k_bounds_final(const float* __restrict__ partial, int n_partials, float* __restrict__ out) {
  Bounds b = empty_bounds();
  for (int i = (int)threadIdx.x; i < n_partials; i += 256) {
    const float* p = partial + (size_t)i * kBoundsWords;
    join(b, p, p + 3, __float_as_uint(p[6]));
  }
  reduce_and_store(b, out);
}

}  // namespace

namespace urtd {

hipError_t skin_vertices(const float* rest_v, const float* rest_n, const int32_t* bone_idx, const float* bone_wgt, const float* bones,
                         int n_bones, int first, int count, float* dst_v, float* dst_n, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  const dim3 grid((unsigned int)(((long long)count + kSkinBlock - 1) / kSkinBlock)), block(kSkinBlock);
  const bool lds = n_bones <= kSkinLdsBones;
  const size_t dyn = lds ? (size_t)n_bones * 48 : 0;
  const int4* ji = (const int4*)bone_idx;
  const float4* wi = (const float4*)bone_wgt;
  if (dst_n) {
    if (lds) hipLaunchKernelGGL((k_skin<true, true>), grid, block, dyn, st, rest_v, rest_n, ji, wi, bones, n_bones, first, count, dst_v, dst_n);
    else hipLaunchKernelGGL((k_skin<true, false>), grid, block, dyn, st, rest_v, rest_n, ji, wi, bones, n_bones, first, count, dst_v, dst_n);
  } else {
    if (lds) hipLaunchKernelGGL((k_skin<false, true>), grid, block, dyn, st, rest_v, rest_n, ji, wi, bones, n_bones, first, count, dst_v, dst_n);
    else hipLaunchKernelGGL((k_skin<false, false>), grid, block, dyn, st, rest_v, rest_n, ji, wi, bones, n_bones, first, count, dst_v, dst_n);
  }
  return hipGetLastError();
}

hipError_t buffer_bounds(const float* v, int first, int count, float* partial, float* out, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  const int blocks = (int)std::min<long long>(kBoundsMaxBlocks, ((long long)count + 255) / 256);
  hipLaunchKernelGGL(k_bounds, dim3(blocks), dim3(256), 0, st, v, first, count, partial);
  hipLaunchKernelGGL(k_bounds_final, dim3(1), dim3(256), 0, st, (const float*)partial, blocks, out);
  return hipGetLastError();
}

}  // namespace urtd
