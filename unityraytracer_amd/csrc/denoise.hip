// denoise.hip — edge-avoiding a-trous wavelet denoiser (Dammertz et al. 2010) over one RGBA32F image, guided by the hit and normal (and
// optionally albedo) feature buffers of urt_render_aov (urt_denoise, include/urt.h, which states the arithmetic).
//
// Two kernels, one pixel per lane, wave64.  A wave covers one 8 x 8 pixel tile and a 256-thread workgroup a 16 x 16 block, as k_aov:
// the 25 taps of a wave are then the same 8 x 8 block shifted by s * (dx, dy), so each tap's loads coalesce into 8 rows of 128 bytes.
//  - k_denoise_pack reads src, normal, hit and albedo once and writes one guide texel per pixel (n.xyz, z; z = -1 marks a pass-through
//    pixel) and the demodulated colour (0 for a pass-through pixel).  A pixel whose demodulated colour is not finite or exceeds 2^120
//    passes through as well (rule 1), so every colour texel a tap loads is finite and at most 2^120 in magnitude.
//  - k_denoise_pass<last> runs pass i with tap spacing s = 2^i: 25 taps, each two float4 loads (colour, guide) at clamped addresses and
//    one exp2f; taps outside the image or on pass-through pixels get weight 0 by a select.  Passes ping-pong between two colour images;
//    the last one remodulates into dst and copies src at pass-through pixels.
// The constants of the exponent are folded on the host (log2(e), 4^i / sigma_c^2, 1 / sigma_n^2) and per pixel (1 / (sigma_z z_p)).
// Domain (include/urt.h): the 1e-4 bound is promised where |c_p / d_p| <= 2^60 and every positive sigma (sigma_color 2^-i for each pass
// i that runs) and z_p lie in [2^-60, 2^60]: there the squares and the folded constants stay normal floats.  Outside that, for every
// finite input, no exponent is NaN (each term is a square times a positive constant; a square or a product that overflows gives
// exp2f(-inf) = 0) and every filtered colour is finite and within the hull of the colours in its reach; only the last pass's
// remodulation c'_p d_p may overflow, at its own pixel.
#include <hip/hip_runtime.h>
#include <float.h>

#include <algorithm>
#include <cmath>

#include "denoise.h"

namespace {

// The folded exponent of one pass: w = h[dx] h[dy] exp2(-(kc |dc|^2 + kn |dn|^2 + (dz kz)^2)), kz = rz / z_p.  A coefficient 0 = the
// term is left out (the test is uniform over the launch).
struct PassConsts {
  float kc, kn, rz;
  int step;
};

struct PixelXY {
  int x, y;
};

// workgroup = 16 x 16 pixels, wave = the 8 x 8 tile (wave & 1, wave >> 1) of it, lane = (lane & 7, lane >> 3) of the tile
__device__ __forceinline__ PixelXY pixel_of_lane() {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  return {(int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3)};
}

// Largest demodulated colour that is filtered (include/urt.h rule 1).  Every pass output is a convex combination of its taps, and its
// float evaluation adds at most ~28 roundings, so from values <= 2^120 no sum of the five passes reaches FLT_MAX.
constexpr float kMaxColor = 0x1p120f;

__device__ __forceinline__ bool finite3(float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

__device__ __forceinline__ float4 demod(const float4* albedo, size_t pix) {
  const float4 a = albedo[pix];
  return make_float4(fmaxf(a.x, 1e-3f), fmaxf(a.y, 1e-3f), fmaxf(a.z, 1e-3f), 0.0f);   // fmaxf: a NaN channel gives 1e-3
}

__global__ __launch_bounds__(256) void k_denoise_pack(const float4* __restrict__ src, const float4* __restrict__ hit,
                                                      const float4* __restrict__ normal, const float4* __restrict__ albedo,
                                                      float4* __restrict__ guide, float4* __restrict__ col, int width, int height) {
  const PixelXY p = pixel_of_lane();
  if (p.x >= width || p.y >= height) return;                     // partial tiles at the right and top edges
  const size_t pix = (size_t)p.y * (size_t)width + (size_t)p.x;
  const float4 c = src[pix], n = normal[pix];
  const float z = hit[pix].w;
  bool surface = n.w != 0.0f && isfinite(z) && z > 0.0f && finite3(c) && finite3(n);
  float4 v = make_float4(c.x, c.y, c.z, 0.0f);
  if (albedo) {
    const float4 d = demod(albedo, pix);
    v = make_float4(c.x / d.x, c.y / d.y, c.z / d.z, 0.0f);
  }
  // the demodulated colour must stay within 2^120: an inf quotient (a finite colour over a small albedo) or a larger value would turn
  // the tap sums of the passes into inf and NaN.  The compare is false for NaN and inf as well.
  surface = surface && fabsf(v.x) <= kMaxColor && fabsf(v.y) <= kMaxColor && fabsf(v.z) <= kMaxColor;
  if (!surface) {
    guide[pix] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    col[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  guide[pix] = make_float4(n.x, n.y, n.z, z);
  col[pix] = v;
}

template <bool kLast>
__global__ __launch_bounds__(256) void k_denoise_pass(const float4* __restrict__ in, const float4* __restrict__ guide,
                                                      float4* out, const float4* src, const float4* __restrict__ albedo,
                                                      int width, int height, PassConsts K) {
  const PixelXY p = pixel_of_lane();
  if (p.x >= width || p.y >= height) return;
  const size_t pix = (size_t)p.y * (size_t)width + (size_t)p.x;
  const float4 g = guide[pix];
  if (!(g.w > 0.0f)) {                                           // pass-through: never filtered; dst gets the src texel bit for bit
    if (kLast) out[pix] = src[pix];
    else out[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const float4 c = in[pix];
  const float kz = fminf(K.rz / g.w, FLT_MAX);                   // 0 when the depth term is off; never inf, so 0 * kz stays 0
  const bool use_c = K.kc > 0.0f, use_n = K.kn > 0.0f, use_z = K.rz > 0.0f;
  constexpr float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const int qy = p.y + K.step * (j - 2);
    const bool in_y = qy >= 0 && qy < height;
    const size_t row = (size_t)min(max(qy, 0), height - 1) * (size_t)width;
#pragma unroll
    for (int i = 0; i < 5; i++) {
      const int qx = p.x + K.step * (i - 2);
      const bool inside = in_y && qx >= 0 && qx < width;
      const size_t q = row + (size_t)min(max(qx, 0), width - 1);
      const float4 gq = guide[q], cq = in[q];                    // finite, |cq| <~ 2^120, for every pixel (pass-through: zeros, z = -1)
      float e = 0.0f;
      if (use_c) {
        const float dr = c.x - cq.x, dg = c.y - cq.y, db = c.z - cq.z;
        e += (dr * dr + dg * dg + db * db) * K.kc;
      }
      if (use_n) {
        const float dx = g.x - gq.x, dy = g.y - gq.y, dz = g.z - gq.z;
        e += (dx * dx + dy * dy + dz * dz) * K.kn;
      }
      if (use_z) {
        const float t = (g.w - gq.w) * kz;
        e += t * t;
      }
      const float w = (inside && gq.w > 0.0f) ? (h[i] * h[j]) * exp2f(-e) : 0.0f;
      sw += w;
      sr += w * cq.x; sg += w * cq.y; sb += w * cq.z;
    }
  }
  const float inv = 1.0f / sw;                                   // sw >= 9/64: the centre tap always counts with exp2(0) = 1
  float4 r = make_float4(sr * inv, sg * inv, sb * inv, 0.0f);
  if (kLast) {
    if (albedo) {
      const float4 d = demod(albedo, pix);
      r.x *= d.x; r.y *= d.y; r.z *= d.z;
    }
    r.w = src[pix].w;
  }
  out[pix] = r;
}

}  // namespace

namespace urtd {

hipError_t launch_denoise(const DenoiseImages& I, const DenoiseSettings& P, hipStream_t st) {
  if (I.width <= 0 || I.height <= 0) return hipSuccess;
  const dim3 grid((unsigned int)((I.width + 15) / 16), (unsigned int)((I.height + 15) / 16));
  if (grid.y > 65535u) return hipErrorInvalidValue;
  const size_t n = (size_t)I.width * (size_t)I.height;
  float4* guide = I.scratch;
  float4* col[2] = {I.scratch + n, I.scratch + 2 * n};
  hipLaunchKernelGGL(k_denoise_pack, grid, dim3(256), 0, st, I.src, I.hit, I.normal, I.albedo, guide, col[0], I.width, I.height);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // exp(-x) = exp2(-x log2 e); the products are taken in double and saturate at FLT_MAX, so that 0 * k stays 0 at the centre tap
  const double log2e = 1.4426950408889634;
  auto sat = [](double v) { return (float)std::min(v, (double)FLT_MAX); };
  const double sc = P.sigma_color, sn = P.sigma_normal, sz = P.sigma_depth;
  for (int i = 0; i < P.iterations; i++) {
    PassConsts K;
    K.kc = sc > 0 ? sat(log2e * std::ldexp(1.0, 2 * i) / (sc * sc)) : 0.0f;     // 1 / (sigma_c 2^-i)^2 = 4^i / sigma_c^2
    K.kn = sn > 0 ? sat(log2e / (sn * sn)) : 0.0f;
    K.rz = sz > 0 ? sat(std::sqrt(log2e) / sz) : 0.0f;                          // (dz / (sigma_z z_p))^2 log2 e = (dz rz / z_p)^2
    K.step = 1 << i;
    const float4* in = col[i & 1];
    if (i + 1 == P.iterations)
      hipLaunchKernelGGL(k_denoise_pass<true>, grid, dim3(256), 0, st, in, guide, I.dst, I.src, I.albedo, I.width, I.height, K);
    else
      hipLaunchKernelGGL(k_denoise_pass<false>, grid, dim3(256), 0, st, in, guide, col[(i + 1) & 1], I.src, I.albedo, I.width,
                         I.height, K);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace urtd
