// morph.hip — k_morph: blend shapes (morph targets) added to the rest pose of a range of vertices (and normals), the stage of a skinned
// mesh that comes before the bones (csrc/skin.hip).  The arithmetic is NORMATIVE (include/urt.h urt_morph_vertices; tests/morph_ref.py
// restates it in numpy): float32, one rounding per operation, evaluated as written, no fma but the two of urt_math.h's dot().  Built
// with -ffp-contract=off like every normative kernel.
#include "morph.h"

#include "../../include/urt_math.h"

namespace {

using namespace urt;
using urtd::kMorphBlock;

// One served vertex per lane, kMorphBlock per workgroup; the 12-byte rows travel dword by dword through LDS as in k_skin (skin.hip), so
// every wave access covers whole cache lines, and only the last block is ragged, whatever `first` is.  A lane walks its own entries, which
// are contiguous (CSR by vertex): the 4-byte target first, the weight through the cache (the table is at most 16 KB and every lane
// reads it), and the entry's 24 bytes of deltas only when the weight is live — a rig has tens of targets and a handful are live.
template <bool kNormals, bool kNormalize>
__global__ __launch_bounds__(kMorphBlock) void k_morph(const float* __restrict__ rest_v, const float* __restrict__ rest_n,
                                                       const int2* __restrict__ ranges, const int* __restrict__ targets,
                                                       const float* __restrict__ deltas, const float* __restrict__ weights, int first,
                                                       int count, float* __restrict__ dst_v, float* __restrict__ dst_n) {
  __shared__ float s_p[3 * kMorphBlock];
  __shared__ float s_n[kNormals ? 3 * kMorphBlock : 1];
  const int tid = (int)threadIdx.x;
  const long long served = (long long)blockIdx.x * kMorphBlock;                      // the block's first vertex, relative to `first`
  const long long left = (long long)count - served;
  const int in_block = left < (long long)kMorphBlock ? (int)left : kMorphBlock;      // >= 1: the grid is ceil(count / kMorphBlock)
  const size_t base = (size_t)((long long)first + served) * 3;
  const int span = 3 * in_block;
  for (int k = tid; k < span; k += kMorphBlock) {
    s_p[k] = rest_v[base + (size_t)k];
    if (kNormals) s_n[k] = rest_n[base + (size_t)k];
  }
  __syncthreads();
  v3 p = mk3(0.0f, 0.0f, 0.0f), n = mk3(0.0f, 0.0f, 0.0f);
  if (tid < in_block) {
    p = mk3(s_p[3 * tid], s_p[3 * tid + 1], s_p[3 * tid + 2]);
    if (kNormals) n = mk3(s_n[3 * tid], s_n[3 * tid + 1], s_n[3 * tid + 2]);
    const int2 r = ranges[(size_t)served + (size_t)tid];
    for (int k = 0; k < r.y; k++) {
      const size_t e = (size_t)r.x + (size_t)k;
      const float w = weights[targets[e]];
      if (w != 0.0f) {                                                               // live (a NaN weight is): else nothing at all
        const float* d = deltas + 6 * e;
        p.x = p.x + w * d[0]; p.y = p.y + w * d[1]; p.z = p.z + w * d[2];
        if (kNormals) { n.x = n.x + w * d[3]; n.y = n.y + w * d[4]; n.z = n.z + w * d[5]; }
      }
    }
    if (kNormals && kNormalize) {
      const float l2 = dot(n, n);
      if (l2 > 0.0f && l2 < __builtin_inff()) n = normalize(n);
    }
  }
  __syncthreads();                                         // every lane has read its rest pose: the span now carries the results
  if (tid < in_block) {
    s_p[3 * tid] = p.x; s_p[3 * tid + 1] = p.y; s_p[3 * tid + 2] = p.z;
    if (kNormals) { s_n[3 * tid] = n.x; s_n[3 * tid + 1] = n.y; s_n[3 * tid + 2] = n.z; }
  }
  __syncthreads();
  for (int k = tid; k < span; k += kMorphBlock) {
    dst_v[base + (size_t)k] = s_p[k];
    if (kNormals) dst_n[base + (size_t)k] = s_n[k];
  }
}

}  // namespace

namespace urtd {

hipError_t morph_vertices(const float* rest_v, const float* rest_n, const int32_t* ranges, const int32_t* targets, const float* deltas,
                          const float* weights, int first, int count, float* dst_v, float* dst_n, bool normalize, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  const dim3 grid((unsigned int)(((long long)count + kMorphBlock - 1) / kMorphBlock)), block(kMorphBlock);
  const int2* rg = (const int2*)ranges;
  if (!dst_n) hipLaunchKernelGGL((k_morph<false, false>), grid, block, 0, st, rest_v, rest_n, rg, targets, deltas, weights, first, count, dst_v, dst_n);
  else if (normalize) hipLaunchKernelGGL((k_morph<true, true>), grid, block, 0, st, rest_v, rest_n, rg, targets, deltas, weights, first, count, dst_v, dst_n);
  else hipLaunchKernelGGL((k_morph<true, false>), grid, block, 0, st, rest_v, rest_n, rg, targets, deltas, weights, first, count, dst_v, dst_n);
  return hipGetLastError();
}

}  // namespace urtd
