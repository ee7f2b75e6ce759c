// bloom.hip — HDR bloom ahead of the tone mapping (urt_bloom): a thresholded copy of the image is taken down a pyramid of halved levels
// with the binomial [1 3 3 1]^2 / 64, brought back up with the bilinear [3 1]^2 / 16 while each level is blended into the one above,
// and added to the image.  include/urt.h states the arithmetic; the library is built with -ffp-contract=off, so every float expression
// below is evaluated with one rounding per operation, in the order written there.  No transcendentals.  The pyramid holds the colour
// channels in float4 texels (w is written 0 and never read for a result).  Every kernel runs 256-thread workgroups over 16 x 16 texels
// of what it writes, four waves of 8 x 8 as csrc/denoise.hip lays them out, and every tap is clamped to its level, so no load leaves it.
//
// k_bloom_down_first     the first downsample, which reads the whole source image and prefilters it: the workgroup's 34 x 34 fine
//                        footprint is prefiltered ONCE per texel on the way into LDS (18.5 KB; 4.5 texels and 9 IEEE divisions a lane
//                        instead of 16 and 32), a second pass writes the 34 x 16 horizontal sums h(row) each pair of vertical
//                        neighbours shares (8.5 KB), and a lane adds four of them, in the header's order.  16 B read per source
//                        texel, 4 B written.  The direct form of k_bloom_down with the prefilter on each tap gave the same bits
//                        and took 19 - 22 % longer together with the composite (profiles/r22_logs/bloom_bench.log; the form is
//                        kept as bloom_direct_first.patch next to that log).
// k_bloom_down           the levels 2..L: one coarse texel per lane, 16 clamped taps of the finer level gathered directly, all loads
//                        in flight at once (L2 serves the 4x overlap between neighbours).  A quarter of the traffic of level 1 and
//                        less: what these launches cost is their latency.
// k_bloom_up             one texel of level l per lane: four clamped taps of level l+1, its own D_l, U_l written over it.  Pointwise in
//                        D_l, so in place.
// k_bloom_composite      one pixel per lane: the src texel, four taps of U_1 (a quarter of the image: L2), one 16-byte store.  dst may be
//                        src: a lane reads its texel before it writes it and nobody else's.
// The exposure of the state is one uniform load in the first downsample; t, cl and k are derived from it on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bloom.h"

namespace {

using urtd::BloomSettings;
using urtd::ExposureState;

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ V3 rgb(float4 p) { return {p.x, p.y, p.z}; }
__device__ __forceinline__ float4 texel(V3 c) { return make_float4(c.x, c.y, c.z, 0.0f); }

struct Knee { float t, cl, k; };

// include/urt.h "exposure": the threshold and the clamp in linear radiance
__device__ __forceinline__ Knee knee_of(const BloomSettings& P, const ExposureState* state) {
  float e = 1.0f;
  if (state) {                                     // (uniform)
    const float s = state->exposure;
    if (s >= 0x1p-60f && s <= 0x1p60f) e = s;      // NaN fails both
  }
  const float t = P.threshold / e;
  return {t, P.clamp / e, t * P.soft_knee};
}

// include/urt.h "prefilter"
__device__ __forceinline__ V3 prefilter(float4 p, Knee K) {
  const float r = p.x > 0.0f ? fminf(p.x, 65504.0f) : 0.0f;
  const float g = p.y > 0.0f ? fminf(p.y, 65504.0f) : 0.0f;
  const float b = p.z > 0.0f ? fminf(p.z, 65504.0f) : 0.0f;
  const float m = fmaxf(fmaxf(r, g), b);
  float q = fminf(fmaxf((m - K.t) + K.k, 0.0f), 2.0f * K.k);
  q = (q * q) / (4.0f * K.k + 1e-5f);
  const float mm = fmaxf(m, 1e-5f);
  float gain = fmaxf(q, m - K.t) / mm;
  gain = gain * fminf(1.0f, K.cl / mm);
  return {r * gain, g * gain, b * gain};
}

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

struct Texel2 { int x, y; };
__device__ __forceinline__ Texel2 tile_texel() {   // 16 x 16 texels a workgroup, 8 x 8 a wave
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  return {(wave & 1) * 8 + (lane & 7), (wave >> 1) * 8 + (lane >> 3)};
}

__device__ __forceinline__ V3 hrow4(V3 a0, V3 a1, V3 a2, V3 a3) { return (a0 + a3) + 3.0f * (a1 + a2); }

__global__ __launch_bounds__(256) void k_bloom_down(const float4* __restrict__ in, float4* __restrict__ out, int win, int hin, int wout,
                                                    int hout) {
  const Texel2 l = tile_texel();
  const int x = (int)blockIdx.x * 16 + l.x, y = (int)blockIdx.y * 16 + l.y;
  if (x >= wout || y >= hout) return;
  int xs[4];
#pragma unroll
  for (int j = 0; j < 4; j++) xs[j] = clampi(2 * x - 1 + j, win - 1);
  V3 h[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const float4* const row = in + (size_t)clampi(2 * y - 1 + j, hin - 1) * (size_t)win;
    h[j] = hrow4(rgb(row[xs[0]]), rgb(row[xs[1]]), rgb(row[xs[2]]), rgb(row[xs[3]]));
  }
  out[(size_t)y * (size_t)wout + (size_t)x] = texel(hrow4(h[0], h[1], h[2], h[3]) * 0.015625f);
}

constexpr int kFoot = 34;                          // fine texels a 16-texel tile reads along an axis: 2 * 16 + 2

__global__ __launch_bounds__(256) void k_bloom_down_first(const float4* __restrict__ in, float4* __restrict__ out, int win, int hin,
                                                          int wout, int hout, const BloomSettings P,
                                                          const ExposureState* __restrict__ state) {
  __shared__ float4 fine[kFoot][kFoot];            // prefiltered; [r][c] is the fine texel (clamp(2*Y0 - 1 + r), clamp(2*X0 - 1 + c))
  __shared__ float4 hsum[kFoot][16];               // h(row) of the 16 coarse columns
  const Knee K = knee_of(P, state);
  const int fx0 = 2 * ((int)blockIdx.x * 16) - 1, fy0 = 2 * ((int)blockIdx.y * 16) - 1;
  for (int i = threadIdx.x; i < kFoot * kFoot; i += 256) {
    const int r = i / kFoot, c = i - r * kFoot;
    const float4 p = in[(size_t)clampi(fy0 + r, hin - 1) * (size_t)win + (size_t)clampi(fx0 + c, win - 1)];
    fine[r][c] = texel(prefilter(p, K));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kFoot * 16; i += 256) {
    const int r = i >> 4, c = i & 15;
    hsum[r][c] = texel(hrow4(rgb(fine[r][2 * c]), rgb(fine[r][2 * c + 1]), rgb(fine[r][2 * c + 2]), rgb(fine[r][2 * c + 3])));
  }
  __syncthreads();
  const Texel2 l = tile_texel();
  const int x = (int)blockIdx.x * 16 + l.x, y = (int)blockIdx.y * 16 + l.y;
  if (x >= wout || y >= hout) return;              // (after the last barrier)
  const V3 d = hrow4(rgb(hsum[2 * l.y][l.x]), rgb(hsum[2 * l.y + 1][l.x]), rgb(hsum[2 * l.y + 2][l.x]), rgb(hsum[2 * l.y + 3][l.x]));
  out[(size_t)y * (size_t)wout + (size_t)x] = texel(d * 0.015625f);
}

// up(a) at the texel (x, y) of the next finer grid; a is wc x hc
__device__ __forceinline__ V3 up_at(const float4* __restrict__ a, int wc, int hc, int x, int y) {
  const int nx = x >> 1, ny = y >> 1;
  const int fx = clampi(nx + ((x & 1) ? 1 : -1), wc - 1), fy = clampi(ny + ((y & 1) ? 1 : -1), hc - 1);
  const float4* const rn = a + (size_t)ny * (size_t)wc;
  const float4* const rf = a + (size_t)fy * (size_t)wc;
  const V3 hn = 3.0f * rgb(rn[nx]) + rgb(rn[fx]);
  const V3 hf = 3.0f * rgb(rf[nx]) + rgb(rf[fx]);
  return (3.0f * hn + hf) * 0.0625f;
}

__global__ __launch_bounds__(256) void k_bloom_up(const float4* __restrict__ coarse, int wc, int hc, float4* __restrict__ level, int w,
                                                  int h, float scatter) {
  const Texel2 l = tile_texel();
  const int x = (int)blockIdx.x * 16 + l.x, y = (int)blockIdx.y * 16 + l.y;
  if (x >= w || y >= h) return;
  const size_t i = (size_t)y * (size_t)w + (size_t)x;
  const V3 d = rgb(level[i]);
  level[i] = texel(d + (up_at(coarse, wc, hc, x, y) - d) * scatter);
}

// (no __restrict__ on src / dst: dst may be src)
__global__ __launch_bounds__(256) void k_bloom_composite(const float4* src, float4* dst, int w, int h, const float4* __restrict__ u1,
                                                         int wc, int hc, float intensity, int only) {
  const Texel2 l = tile_texel();
  const int x = (int)blockIdx.x * 16 + l.x, y = (int)blockIdx.y * 16 + l.y;
  if (x >= w || y >= h) return;
  const size_t i = (size_t)y * (size_t)w + (size_t)x;
  float4 p = src[i];
  const V3 glow = up_at(u1, wc, hc, x, y) * intensity;
  p.x = only ? glow.x : p.x + glow.x;
  p.y = only ? glow.y : p.y + glow.y;
  p.z = only ? glow.z : p.z + glow.z;
  dst[i] = p;                                      // alpha: the bits that were loaded
}

dim3 tiles(int w, int h) { return dim3((unsigned int)((w + 15) / 16), (unsigned int)((h + 15) / 16)); }

}  // namespace

namespace urtd {

BloomLevels bloom_levels(int width, int height, int levels) {
  BloomLevels B{};
  B.w[0] = width;
  B.h[0] = height;
  for (int l = 1; l <= levels && l <= kBloomMaxLevels; l++) {
    B.w[l] = (B.w[l - 1] + 1) >> 1;
    B.h[l] = (B.h[l - 1] + 1) >> 1;
    B.offset[l] = B.texels;
    B.texels += (size_t)B.w[l] * (size_t)B.h[l];
    B.L = l;
    if (B.w[l] == 1 && B.h[l] == 1) break;
  }
  return B;
}

hipError_t launch_bloom(const float4* src, float4* dst, int width, int height, const BloomSettings& P, const ExposureState* state,
                        float4* pyramid, hipStream_t st) {
  if (width < 1 || height < 1 || width > kBloomMaxExtent || height > kBloomMaxExtent || (height + 15) / 16 > 65535 || P.levels < 1)
    return hipErrorInvalidValue;
  const BloomLevels B = bloom_levels(width, height, P.levels);
  float4* const D1 = pyramid + B.offset[1];
  hipLaunchKernelGGL(k_bloom_down_first, tiles(B.w[1], B.h[1]), dim3(256), 0, st, src, D1, width, height, B.w[1], B.h[1], P, state);
  for (int l = 2; l <= B.L; l++)
    hipLaunchKernelGGL(k_bloom_down, tiles(B.w[l], B.h[l]), dim3(256), 0, st, (const float4*)(pyramid + B.offset[l - 1]),
                       pyramid + B.offset[l], B.w[l - 1], B.h[l - 1], B.w[l], B.h[l]);
  for (int l = B.L - 1; l >= 1; l--)
    hipLaunchKernelGGL(k_bloom_up, tiles(B.w[l], B.h[l]), dim3(256), 0, st, (const float4*)(pyramid + B.offset[l + 1]), B.w[l + 1],
                       B.h[l + 1], pyramid + B.offset[l], B.w[l], B.h[l], P.scatter);
  hipLaunchKernelGGL(k_bloom_composite, tiles(width, height), dim3(256), 0, st, src, dst, width, height, (const float4*)D1, B.w[1], B.h[1],
                     P.intensity, P.flags & 1);
  return hipGetLastError();
}

}  // namespace urtd
