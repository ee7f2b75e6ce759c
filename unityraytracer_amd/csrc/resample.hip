// resample.hip — the resampling step of the temporal pipeline on the GPU: the ordered stream compaction of a count texture into a
// urt_PathPixel list (urt_select_pixels) and the sparse AdditionShader blend of a sample list (urt_blend_samples).  include/urt.h states
// the semantics; the library is built with -ffp-contract=off, so the blend below is evaluated with one rounding per operation, as
// k_blit_add_history's is.
//
// The compaction is three launches, none of which waits for another workgroup (no look-back, no flags, no spin; no atomics, which
// would lose the order):
//   k_select_count  a 256-thread workgroup takes kSelectChunk consecutive texels, each of its four waves 512 consecutive ones in
//                   kSelectRounds rounds of 64: one dword load per texel (the .x of the 16-byte count texel), one ballot and one popcount
//                   per round; the four wave sums meet in LDS and the workgroup writes ONE count;
//   k_select_scan   one workgroup turns the block counts into their exclusive prefix sums, 2048 per trip (eight per thread, a wave scan
//                   by shuffles and the four wave sums in LDS), and writes the grand total behind them;
//   k_select_write  recomputes the ballots; a lane's rank is the block's base + the sums of the waves before its own (LDS) + the rounds
//                   before its own + popcount(ballot & lanes below it), and it stores {x, y} with one 8-byte store when rank < capacity.
// The texel index is a size_t (16 bytes per texel: byte offsets pass 2^32 at 2160p x 32); the host keeps width * height <= 2^31 - 1, so
// x and y come from one 32-bit division.
// k_blend_samples: one thread per list entry: an 8-byte load of the pixel, a 16-byte load of the sample, a float4 read-modify-write on
// dst and on count.  The per-pixel function restates reproject.hip's blend with `weight` in place of 1.0f (that file is not touched: its
// generated code stays what it is); with weight == 1.0f the two are the same operations in the same order.
#include <hip/hip_runtime.h>

#include "resample.h"

namespace {

using urtd::kSelectChunk;
using urtd::kSelectRounds;

constexpr int kScanItems = 8;                      // block counts per thread and trip of k_select_scan
constexpr int kScanStride = 256 * kScanItems;

// The selection ballots of this wave's kSelectRounds x 64 consecutive texels from `first` on (round r: texel first + 64 r + lane);
// returns how many of them are selected.  A texel is selected when !(count.x >= below): NaN and negative counts are, +inf is not.
__device__ __forceinline__ unsigned int wave_select(const float4* __restrict__ count, size_t first, size_t n_texels, float below, int lane,
                                                    unsigned long long (&ballots)[kSelectRounds]) {
  float c[kSelectRounds];
  bool in[kSelectRounds];
#pragma unroll
  for (int r = 0; r < kSelectRounds; r++) {        // all loads first: eight independent dwords in flight per lane
    const size_t i = first + (size_t)(r * 64 + lane);
    in[r] = i < n_texels;
    c[r] = in[r] ? count[i].x : 0.0f;
  }
  unsigned int n = 0;
#pragma unroll
  for (int r = 0; r < kSelectRounds; r++) {
    ballots[r] = __ballot(in[r] && !(c[r] >= below));
    n += (unsigned int)__popcll(ballots[r]);
  }
  return n;
}

__global__ __launch_bounds__(256) void k_select_count(const float4* __restrict__ count, size_t n_texels, float below,
                                                      unsigned int* __restrict__ block_count) {
  __shared__ unsigned int wave_sum[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned long long ballots[kSelectRounds];
  const size_t first = (size_t)blockIdx.x * (size_t)kSelectChunk + (size_t)(wave * 64 * kSelectRounds);
  const unsigned int n = wave_select(count, first, n_texels, below, lane, ballots);
  if (lane == 0) wave_sum[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// counts[0 .. n_blocks) -> their exclusive prefix sums, counts[n_blocks] = the total.  One workgroup; ceil(n_blocks / 2048) trips.
__global__ __launch_bounds__(256) void k_select_scan(unsigned int* __restrict__ counts, unsigned int n_blocks) {
  __shared__ unsigned int wave_sum[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned int carry = 0;
  for (unsigned int base = 0; base < n_blocks; base += (unsigned int)kScanStride) {
    const unsigned int first = base + threadIdx.x * (unsigned int)kScanItems;
    unsigned int v[kScanItems], sum = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
      v[k] = first + k < n_blocks ? counts[first + k] : 0u;
      sum += v[k];
    }
    unsigned int inc = sum;                        // inclusive scan of the threads' sums over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned int o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    unsigned int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const unsigned int s = wave_sum[w];
      if (w < wave) before += s;
      total += s;
    }
    unsigned int run = carry + before + (inc - sum);
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
      if (first + k < n_blocks) counts[first + k] = run;
      run += v[k];
    }
    carry += total;
    __syncthreads();                               // wave_sum is written again by the next trip
  }
  if (threadIdx.x == 0) counts[n_blocks] = carry;
}

__global__ __launch_bounds__(256) void k_select_write(const float4* __restrict__ count, unsigned int width, size_t n_texels, float below,
                                                      const unsigned int* __restrict__ block_base, int2* __restrict__ pixels,
                                                      unsigned int capacity) {
  __shared__ unsigned int wave_sum[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned long long ballots[kSelectRounds];
  const size_t first = (size_t)blockIdx.x * (size_t)kSelectChunk + (size_t)(wave * 64 * kSelectRounds);
  const unsigned int n = wave_select(count, first, n_texels, below, lane, ballots);
  if (lane == 0) wave_sum[wave] = n;
  __syncthreads();
  unsigned int rank = block_base[blockIdx.x];
  for (int w = 0; w < wave; w++) rank += wave_sum[w];
  if (n == 0 || rank >= capacity) return;          // wave-uniform, after the workgroup's only barrier
  const unsigned long long below_me = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < kSelectRounds; r++) {
    const unsigned long long b = ballots[r];
    if ((b >> lane) & 1ull) {
      const unsigned int k = rank + (unsigned int)__popcll(b & below_me);
      if (k < capacity) {
        const unsigned int i = (unsigned int)(first + (size_t)(r * 64 + lane));   // < n_texels <= 2^31 - 1
        pixels[k] = make_int2((int)(i % width), (int)(i / width));
      }
    }
    rank += (unsigned int)__popcll(b);
  }
}

// the sample count a blend of `weight` frame-equivalents uses: 0 for a count that is not finite or negative, else the count, capped so
// that the new count stays within max_history
__device__ __forceinline__ float blend_history(float n, float max_history, float weight) {
  if (!isfinite(n) || n < 0.0f) return 0.0f;
  return max_history > 0.0f ? fminf(n, fmaxf(max_history - weight, 0.0f)) : n;
}

// reproject.hip's blend with `weight` in place of 1.0f
__device__ __forceinline__ float4 blend_weighted(float4 c, float4 t, float s, float weight) {
  const float a = weight / (s + weight);
  const float ia = 1.0f - a;
  c.x = t.x * a + c.x * ia;
  c.y = t.y * a + c.y * ia;
  c.z = t.z * a + c.z * ia;
  c.w = a * a + c.w * ia;
  return c;
}

__global__ __launch_bounds__(256) void k_blend_samples(const int2* __restrict__ pixels, const float4* __restrict__ samples, unsigned int n,
                                                       float weight, float4* __restrict__ dst, float4* __restrict__ count, int width,
                                                       int height, float max_history) {
  const unsigned int i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int2 p = pixels[i];
  if (p.x < 0 || p.x >= width || p.y < 0 || p.y >= height) return;   // not a pixel of dst: skipped, nothing is written
  const size_t q = (size_t)p.y * (size_t)width + (size_t)p.x;
  const float4 t = samples[i];
  const float4 cn = count[q];
  const float s = blend_history(cn.x, max_history, weight);
  dst[q] = blend_weighted(dst[q], t, s, weight);
  count[q] = make_float4(s + weight, 0.0f, 0.0f, 0.0f);
}

}  // namespace

namespace urtd {

hipError_t launch_select_count(const float4* count, size_t n_texels, float below, unsigned int* scratch, hipStream_t st) {
  const size_t blocks = select_blocks(n_texels);
  if (n_texels > 0x7fffffffull) return hipErrorInvalidValue;
  if (blocks > 0) hipLaunchKernelGGL(k_select_count, dim3((unsigned int)blocks), dim3(256), 0, st, count, n_texels, below, scratch);
  hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(256), 0, st, scratch, (unsigned int)blocks);
  return hipGetLastError();
}

hipError_t launch_select_write(const float4* count, int width, size_t n_texels, float below, const unsigned int* scratch, int2* pixels,
                               int capacity, hipStream_t st) {
  const size_t blocks = select_blocks(n_texels);
  if (n_texels > 0x7fffffffull || width <= 0) return hipErrorInvalidValue;
  if (blocks == 0 || capacity <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_select_write, dim3((unsigned int)blocks), dim3(256), 0, st, count, (unsigned int)width, n_texels, below, scratch,
                     pixels, (unsigned int)capacity);
  return hipGetLastError();
}

hipError_t launch_blend_samples(const int2* pixels, const float4* samples, int n, float weight, float4* dst, float4* count, int width,
                                int height, float max_history, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const unsigned int blocks = ((unsigned int)n + 255u) / 256u;
  hipLaunchKernelGGL(k_blend_samples, dim3(blocks), dim3(256), 0, st, pixels, samples, (unsigned int)n, weight, dst, count, width, height,
                     max_history);
  return hipGetLastError();
}

}  // namespace urtd
