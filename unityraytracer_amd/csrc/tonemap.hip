// tonemap.hip — the last image-space stage ahead of the 8-bit present: a metered exposure (urt_auto_exposure) and a tone-mapping
// operator (urt_tonemap) that brings linear HDR radiance into [0, 1] before present.hip's sRGB table clamps it.  include/urt.h states the
// arithmetic; the library is built with -ffp-contract=off, so every float expression below is evaluated with one rounding per operation,
// as written there.  No transcendentals: the luminance is binned by the top bits of its float (four bins per stop) and the metered
// luminance is read back piecewise-linearly in bit space.
//
// k_luminance_histogram  HBM-bound: 16 B per texel (32 B with a count texture), dwordx4 loads, a grid capped at kExposureMaxBlocks
//                        workgroups that stride over the image, kHistUnroll independent texels in flight per lane.  All counting is
//                        in integers, so any order of the additions gives the same words.  The 256 bins are privatised in LDS, ONE
//                        COPY PER WAVE (4 KB a workgroup): a wave's LDS adds never meet another wave's.  A sky-dominated image puts
//                        most of a wave's 64 texels into one bin, which 64 ds_add on one address would serialise; so the lanes that
//                        share the bin of the wave's first valid lane are folded by a ballot into one add of their popcount, and only
//                        the others add for themselves.  At the end each thread sums one bin over the four copies and adds it, when
//                        it is not zero, with one global atomic to one of kExposureCopies accumulators in the context's scratch
//                        (workgroup b: copy b % kExposureCopies — a thousand adds on ONE word cost more than the whole image's
//                        loads, and the copies spread them; profiles/r20_logs/hist_sweep.log has the grid, the unroll and the number
//                        of copies swept); skipped texels are counted by ballots in a wave-uniform register.
// k_exposure_resolve     one 256-thread workgroup, one bin per thread: sums the accumulators and ZEROES them for the next call (they
//                        are zero whenever no call is in flight: no memset per call), stores hist, then a prefix sum of the bins
//                        (wave scan by shuffles, the four wave sums in LDS), the overlap of each bin's rank interval with the trimmed
//                        window in 64-bit integers, a 64-bit sum of bin * kept, and thread 0 finishes the float arithmetic and
//                        writes the scalars of the state.  No host round trip.
// k_tonemap              one pixel per lane, 16 B in, 16 B out, in place when dst == src; the state's exposure is one uniform load.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tonemap.h"

namespace {

using urtd::ExposureSettings;
using urtd::ExposureState;
using urtd::kExposureBins;
using urtd::kExposureCopies;
using urtd::kExposureWords;
using urtd::TonemapSettings;

constexpr int kHistUnroll = 4;                     // texels per lane and trip of k_luminance_histogram

static_assert(sizeof(ExposureState) == 1040, "include/urt.h urt_ExposureState");
static_assert(kExposureBins == 256, "one bin per thread of the 256-thread workgroups");

template <int kUnroll>
__global__ __launch_bounds__(256) void k_luminance_histogram(const float4* __restrict__ src, const float4* __restrict__ count,
                                                             unsigned int n_texels, unsigned int* __restrict__ accum, unsigned int n_copies) {
  __shared__ unsigned int bins[4][kExposureBins];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int w = 0; w < 4; w++) bins[w][threadIdx.x] = 0u;
  __syncthreads();
  unsigned int* const mine = bins[wave];
  unsigned int skipped = 0;                        // wave-uniform
  const unsigned int stride = gridDim.x * 256u;    // <= 2^18; n_texels <= 2^31 - 1: no index below wraps
  for (unsigned int first = blockIdx.x * 256u + (unsigned int)(wave * 64); first < n_texels; first += stride * (unsigned int)kUnroll) {
    float4 p[kUnroll];
    float c[kUnroll];
    bool in[kUnroll];
#pragma unroll
    for (int r = 0; r < kUnroll; r++) {            // all loads first
      const unsigned int i = first + (unsigned int)r * stride + (unsigned int)lane;
      in[r] = i < n_texels;
      p[r] = in[r] ? src[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      c[r] = (in[r] && count) ? count[i].x : 1.0f;
    }
#pragma unroll
    for (int r = 0; r < kUnroll; r++) {
      const float Y = (0.2126f * p[r].x + 0.7152f * p[r].y) + 0.0722f * p[r].z;
      const bool ok = in[r] && Y > 0.0f && Y <= 3.402823466e+38f && c[r] > 0.0f;   // NaN fails every comparison
      skipped += (unsigned int)__popcll(__ballot(in[r] && !ok));
      const int k = min(max((int)(__float_as_uint(Y) >> 21) - 380, 0), kExposureBins - 1);
      const unsigned long long valid = __ballot(ok);
      if (valid) {                                 // (uniform)
        const int leader = __ffsll((long long)valid) - 1;
        const int k0 = __shfl(k, leader);
        const unsigned long long same = __ballot(ok && k == k0);
        if (lane == leader) atomicAdd(&mine[k0], (unsigned int)__popcll(same));
        else if (ok && k != k0) atomicAdd(&mine[k], 1u);
      }
    }
  }
  __syncthreads();
  const unsigned int v = (bins[0][threadIdx.x] + bins[1][threadIdx.x]) + (bins[2][threadIdx.x] + bins[3][threadIdx.x]);
  unsigned int* const out = accum + (blockIdx.x % n_copies) * (unsigned int)kExposureWords;
  if (v) atomicAdd(&out[threadIdx.x], v);
  if (lane == 0 && skipped) atomicAdd(&out[kExposureBins], skipped);
}

__global__ __launch_bounds__(256) void k_exposure_resolve(unsigned int* __restrict__ accum, unsigned int n_copies,
                                                          ExposureState* __restrict__ state, const ExposureSettings P) {
  __shared__ unsigned int wave_count[4];
  __shared__ unsigned long long wave_sum[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned int h = 0, skipped = 0;
  for (unsigned int c = 0; c < n_copies; c++) {    // this call's counts, and zeros for the next call
    unsigned int* const a = accum + c * (unsigned int)kExposureWords;
    h += a[threadIdx.x];
    a[threadIdx.x] = 0u;
    if (threadIdx.x == 0) { skipped += a[kExposureBins]; a[kExposureBins] = 0u; }
  }
  state->hist[threadIdx.x] = h;
  unsigned int inc = h;                            // inclusive scan over the wave; the total is <= 2^31 - 1
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wave_count[wave] = inc;
  __syncthreads();
  unsigned int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const unsigned int s = wave_count[w];
    if (w < wave) before += s;
    total += s;
  }
  // the samples of this bin have the ranks [prefix, prefix + h); the window keeps [lo, hi)
  const unsigned long long T = total, prefix = (unsigned long long)before + (unsigned long long)(inc - h);
  const unsigned long long lo = T * (unsigned long long)P.low_permille / 1000ull, hi = T * (unsigned long long)P.high_permille / 1000ull;
  const unsigned long long a = prefix > lo ? prefix : lo, b = prefix + h < hi ? prefix + h : hi;
  unsigned long long sum = b > a ? (unsigned long long)threadIdx.x * (b - a) : 0ull;   // <= 255 * 2^31
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d);
  if (lane == 0) wave_sum[wave] = sum;
  __syncthreads();
  if (threadIdx.x != 0) return;
  state->counted = total;
  state->skipped = skipped;
  const unsigned long long M = hi - lo;
  if (M == 0ull) return;                           // nothing metered: exposure and target stay
  const unsigned long long q = (((wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3])) * 256ull) / M;   // <= 255 * 256
  const float L = __uint_as_float((380u << 21) + ((unsigned int)q << 13) + (1u << 20));
  const float target = fminf(fmaxf(P.key / L, P.min_exposure), P.max_exposure);
  const float prev = state->exposure;
  float e = target;
  if (prev > 0.0f && prev <= 3.402823466e+38f && !(P.rate >= 1.0f)) e = prev + (target - prev) * P.rate;
  state->target = target;
  state->exposure = e;
}

__device__ __forceinline__ float tonemap_channel(float c, float e, float w2, int op) {
  float x = c * e;
  if (!(x > 0.0f)) x = 0.0f;                       // NaN, negatives, -0
  else x = fminf(x, 65504.0f);
  if (op == 1) return fminf((x * (1.0f + x / w2)) / (1.0f + x), 1.0f);                                     // URT_TONEMAP_REINHARD
  if (op == 2) return fminf((x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f), 1.0f);          // URT_TONEMAP_ACES
  return x;                                                                                                // URT_TONEMAP_LINEAR
}

// (no __restrict__: dst may be src)
__global__ __launch_bounds__(256) void k_tonemap(const float4* src, float4* dst, size_t n_texels, const TonemapSettings P,
                                                 const ExposureState* state) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_texels) return;
  float e = P.exposure;
  if (state) {                                     // (uniform)
    const float s = state->exposure;
    if (s > 0.0f && s <= 3.402823466e+38f) e = s * P.exposure;
  }
  const float w2 = P.white * P.white;
  float4 p = src[i];
  p.x = tonemap_channel(p.x, e, w2, P.op);
  p.y = tonemap_channel(p.y, e, w2, P.op);
  p.z = tonemap_channel(p.z, e, w2, P.op);
  dst[i] = p;                                      // alpha: the bits that were loaded
}

}  // namespace

namespace urtd {

hipError_t launch_auto_exposure(const float4* src, const float4* count, size_t n_texels, const ExposureSettings& P, unsigned int* accum,
                                ExposureState* state, hipStream_t st) {
  if (n_texels > 0x7fffffffull) return hipErrorInvalidValue;
  const size_t blocks = (n_texels + 255) / 256;
  if (blocks > 0)
    hipLaunchKernelGGL(k_luminance_histogram<kHistUnroll>,
                       dim3((unsigned int)(blocks < (size_t)kExposureMaxBlocks ? blocks : (size_t)kExposureMaxBlocks)), dim3(256), 0, st, src, count,
                       (unsigned int)n_texels, accum, (unsigned int)kExposureCopies);
  hipLaunchKernelGGL(k_exposure_resolve, dim3(1), dim3(256), 0, st, accum, (unsigned int)kExposureCopies, state, P);
  return hipGetLastError();
}

hipError_t launch_tonemap(const float4* src, float4* dst, size_t n_texels, const TonemapSettings& P, const ExposureState* state,
                          hipStream_t st) {
  if (n_texels == 0) return hipSuccess;
  const size_t blocks = (n_texels + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tonemap, dim3((unsigned int)blocks), dim3(256), 0, st, src, dst, n_texels, P, state);
  return hipGetLastError();
}

}  // namespace urtd
