// bounds_device.h — the min / max reduction of a 256-thread workgroup, as csrc/skin.hip (k_bounds) and csrc/object_bvh.hip (the mesh leaf
// boxes) share it: per lane, then by shuffles inside the wave, then through LDS across the four waves.  Device code only.  Private.
#pragma once
#include <hip/hip_runtime.h>

namespace urtd {

struct Bounds { float lo[3], hi[3]; unsigned int n; };

__device__ __forceinline__ Bounds empty_bounds() {
  Bounds b;
  for (int c = 0; c < 3; c++) { b.lo[c] = __builtin_inff(); b.hi[c] = -__builtin_inff(); }
  b.n = 0;
  return b;
}

// A NaN fails both comparisons: it takes no part in that component's min or max.
__device__ __forceinline__ void join(Bounds& b, const float lo[3], const float hi[3], unsigned int n) {
  for (int c = 0; c < 3; c++) { b.lo[c] = lo[c] < b.lo[c] ? lo[c] : b.lo[c]; b.hi[c] = hi[c] > b.hi[c] ? hi[c] : b.hi[c]; }
  b.n += n;
}

// The workgroup's union, valid in its first lane: lanes by shuffles, the waves through LDS.  Min and max are exact, so the order does not
// matter.  Every lane of the workgroup calls it (it holds a barrier).
__device__ __forceinline__ Bounds reduce_block(Bounds b) {
  for (int off = 32; off > 0; off >>= 1) {
    float lo[3], hi[3];
    for (int c = 0; c < 3; c++) { lo[c] = __shfl_xor(b.lo[c], off, 64); hi[c] = __shfl_xor(b.hi[c], off, 64); }
    const unsigned int n = (unsigned int)__shfl_xor((int)b.n, off, 64);
    join(b, lo, hi, n);
  }
  __shared__ float s_lo[4][3], s_hi[4][3];
  __shared__ unsigned int s_cnt[4];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  if (lane == 0) { for (int c = 0; c < 3; c++) { s_lo[wave][c] = b.lo[c]; s_hi[wave][c] = b.hi[c]; } s_cnt[wave] = b.n; }
  __syncthreads();
  Bounds r = empty_bounds();
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) join(r, s_lo[w], s_hi[w], s_cnt[w]);
  return r;
}

// ... written by the first lane to out[8]: min.xyz, max.xyz, the count (as bits), 0
__device__ __forceinline__ void reduce_and_store(Bounds b, float* __restrict__ out) {
  const Bounds r = reduce_block(b);
  if (threadIdx.x == 0) {
    out[0] = r.lo[0]; out[1] = r.lo[1]; out[2] = r.lo[2]; out[3] = r.hi[0]; out[4] = r.hi[1]; out[5] = r.hi[2];
    out[6] = __uint_as_float(r.n); out[7] = 0.0f;
  }
}

}  // namespace urtd
